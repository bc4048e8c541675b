#!/usr/bin/env python3
"""Loop closing (csrc/loop_close.hip, csrc/pose_graph.cpp) by the
numbers, run by hand (not part of bench.py), at 640x480:

  (1) kernels   k_loop_signature timed with HIP events for 512 frames and for 1
                frame per call (us per frame, achieved read bandwidth at
                3 B/px); youth_loop_distances (upload, k_loop_distance,
                download) for 512 queries and for 1 query against 512 keyframes
  (2) gates     every pair of the C5 keyframes (every 10th frame, 100 of them)
                at least two keyframes apart, verified forward and backward,
                with DEFAULT_FLAGS and SURVEY_FLAGS noise: per gate the largest
                value over true pairs and the smallest over wrong pairs.
                A true pair: its forward result is within 0.05 degrees and
                1 mm of the true relative pose.  A wrong pair: more than
                1 degree or 10 mm off.  Also the prefilter distance per cell
                of both groups, how many revisits by pose (300 frames or more
                apart, within 0.15 m and 8 degrees) align to a true pair, and
                which pairs the default gates accept.
  (3) C5        the 1000-frame sequence tracked depth-only and with colour,
                keyframes picked as the drop-in picks them (0.10 m / 10 deg),
                stored and closed in order; the error of the composed
                trajectory against T_wc at frames 627, 800 and 999 before and
                after optimising and re-hanging; close time per keyframe

  (4) c5map     (on request only) C5 tracked with colour as in (3), every frame
                integrated into a voxel map at 100 voxels per metre with its
                tracked pose, the frames kept on the device in chunks of 64 as
                the drop-in keeps them; then moved to the corrected trajectory
                (youth_map_move_device per chunk) and compacted.  Reported: the
                Jaccard index of the map's voxel key set, before and after,
                against the map integrated with the ground-truth poses, and the
                time of the re-integration

With --levels SPEC (`auto`, or stride:iterations items such as 8:10,1:10 ending
at stride 1) parts (2) and (3) run twice in the same process,
without a schedule and with the closer verifying through that one, and report
both ("none" and "levels"; in (3) the tracking is shared, the rows with the
schedule are named depth+levels and rgbd+levels).

The last line is one JSON object.
usage: python tools/loop_bench.py [kernels] [gates] [c5] [c5track] [c5map] [dump=DIR] [--levels SPEC]
       [--track-levels SPEC]   (c5: a third trajectory tracked by the streaming tracker with its own
       schedule; c5track, on request only: C5's tracking errors alone, without and with that schedule)
(default: the first three; dump=DIR also writes every verified pair and every loop edge as
JSON files into DIR)"""
import json
import os
import sys
import time

import torch  # noqa: F401  (first: shared HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-rgbd_amd"))
import numpy as np  # noqa: E402

import youth_icp  # noqa: E402
import youth_loop  # noqa: E402
import youth_map  # noqa: E402
import youth_rgbd  # noqa: E402
import youth_synth  # noqa: E402

W, H = 640, 480
READ_CEILING = 6.48e12   # B/s, the measured read-stream ceiling


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3),
            "max": round(float(np.max(v)), 3)}


def pose_error(T, T_gt):
    D = np.linalg.inv(T_gt) @ T
    v = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    ang = np.degrees(np.arctan2(np.linalg.norm(v), 0.5 * (np.trace(D[:3, :3]) - 1.0)))
    return float(ang), float(np.linalg.norm(D[:3, 3]) * 1000.0)


# -------------------------------------------------------------------- kernels --
def kernel_times(rounds=3, reps=5):
    fr, _, rgb = youth_synth.sequence_rgb(0, 8, W, H)
    gray = youth_synth.luma(rgb)
    s = torch.cuda.Stream()
    out = {}
    for n in (512, 1):
        d = torch.from_numpy(np.ascontiguousarray(fr[np.arange(n) % 8])).cuda()
        g = torch.from_numpy(np.ascontiguousarray(gray[np.arange(n) % 8])).cuda()
        sig = torch.zeros((n, 300), dtype=torch.int32, device="cuda")
        calls = 4 if n > 1 else 64
        t = []
        for r in range(rounds + 1):                    # round 0 warms up
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(calls):
                    youth_loop.signature_device(d.data_ptr(), g.data_ptr(), n, W, H, sig.data_ptr(),
                                                stream=s.cuda_stream)
                e1.record(s)
                e1.synchronize()
                if r > 0:
                    t.append(e0.elapsed_time(e1) / (calls * n) * 1e3)
        st = stats(t)
        st["TBps"] = round(3.0 * W * H / (st["median"] * 1e-6) / 1e12, 3)
        st["of_read_ceiling"] = round(st["TBps"] * 1e12 / READ_CEILING, 3)
        out[f"signature_us_per_frame_batch{n}"] = st
        print(f"signature, {n:3d} frames per call: {st}", flush=True)
        del d, g, sig
    sigs = np.random.default_rng(0).integers(0, 1 << 32, (512, 300), dtype=np.uint64).astype(np.uint32)
    with youth_loop.LoopCloser(W, H, 512) as lc:
        for k in range(512):
            lc.add_keyframe(fr[k % 8], rgb[k % 8], np.eye(4))
        for nq in (512, 1):
            t = []
            for r in range(rounds * reps + 1):
                t0 = time.perf_counter()
                lc.distances(sigs[:nq])
                if r > 0:
                    t.append((time.perf_counter() - t0) / nq * 1e6)
            out[f"distances_call_us_per_query_nq{nq}_vs_512"] = stats(t)
            print(f"distances call, {nq:3d} queries x 512 keyframes: {stats(t)} us per query", flush=True)
    return out


# ---------------------------------------------------------------------- gates --
def gate_table(flags, name, step=10, n_kf=100, levels=None):
    frames = [k * step for k in range(n_kf)]
    fr, X, rgb = [], [], []
    for f in frames:
        a, T, c = youth_synth.sequence_rgb(f, 1, W, H, flags=flags)
        fr.append(a[0]), X.append(T[0]), rgb.append(c[0])
    rows = []
    with youth_loop.LoopCloser(W, H, 17, min_gap=1, max_candidates=16, max_cell_dist=65535) as lc:
        lc.set_levels(levels)
        for q in range(2, n_kf):
            if q % 10 == 0:
                print(f"gates, {name}: keyframe {q} of {n_kf}", file=sys.stderr, flush=True)
            for c0 in range(0, q - 1, 16):             # candidates 0 .. q - 2, 16 at a time
                ks = list(range(c0, min(c0 + 16, q - 1)))
                lc.clear()
                for k in ks:
                    lc.add_keyframe(fr[k], rgb[k], X[k])
                lc.add_keyframe(fr[q], rgb[q], X[q])
                idx, dist = lc.candidates(len(ks), 16)
                per_cell = {int(i): int(dv) / 300.0 for i, dv in zip(idx, dist)}
                lc.close(len(ks))
                for e in lc.last_verified():
                    k = ks[int(e["i"])]
                    gt = np.linalg.inv(X[k]) @ X[q]
                    off = pose_error(np.eye(4), gt)
                    err = pose_error(e["Z"], gt)
                    rows.append(dict(k=k, q=q, off=off, err=err, cell=per_cell.get(int(e["i"])), w=float(e["w"]),
                                     overlap=float(e["overlap"]), rms=float(e["gray_rms"]),
                                     fb_deg=float(e["fb_rot_deg"]), fb_mm=float(e["fb_trans_m"]) * 1e3))
    # by the accuracy of the forward result: a true pair meets the bar an edge is
    # tested against (0.05 deg / 1 mm); a wrong pair would bend the graph; a
    # pair whose verification applied no update (fb exactly 0, status not 0) is
    # rejected by its status and left out of the wrong pairs' gate values
    true = [r for r in rows if r["err"][0] <= 0.05 and r["err"][1] <= 1.0]
    wrong = [r for r in rows if (r["err"][0] > 1.0 or r["err"][1] > 10.0) and r["fb_mm"] > 0.0]
    revisit = [r for r in rows if (r["q"] - r["k"]) * step >= 300 and r["off"][0] <= 8.0 and r["off"][1] <= 150.0]

    def span(group, key, pick):
        v = [r[key] for r in group if r[key] is not None and np.isfinite(r[key])]
        return round(float(pick(v)), 4) if v else None

    acc = [r for r in rows if r["w"] == 1.0]           # the library's own decision
    res = {
        "pairs": len(rows), "true_pairs": len(true), "wrong_pairs": len(wrong),
        "revisits_by_pose": len(revisit), "revisits_aligned_true": sum(1 for r in revisit if r in true),
        "cell_dist": {"true_max": span(true, "cell", max), "wrong_min": span(wrong, "cell", min)},
        "overlap": {"true_min": span(true, "overlap", min), "wrong_max": span(wrong, "overlap", max)},
        "gray_rms": {"true_max": span(true, "rms", max), "wrong_min": span(wrong, "rms", min),
                     "all_pairs_min": span(rows, "rms", min)},
        "fb_deg": {"true_max": span(true, "fb_deg", max), "wrong_min": span(wrong, "fb_deg", min)},
        "fb_mm": {"true_max": span(true, "fb_mm", max), "wrong_min": span(wrong, "fb_mm", min)},
        "accepted": len(acc), "accepted_true": sum(1 for r in acc if r in true),
        "accepted_wrong": sum(1 for r in acc if r in wrong),
        "accepted_not_true": [dict(k=r["k"], q=r["q"], err=[round(v, 4) for v in r["err"]],
                                   overlap=round(r["overlap"], 3), rms=round(r["rms"], 3),
                                   fb_deg=round(r["fb_deg"], 4), fb_mm=round(r["fb_mm"], 3))
                              for r in acc if r not in true],
        "accepted_error_max_deg_mm": [span([dict(v=r["err"][0]) for r in acc], "v", max),
                                      span([dict(v=r["err"][1]) for r in acc], "v", max)],
    }
    print(f"gates, {name}: {res}", flush=True)
    if DUMP:
        with open(os.path.join(DUMP, f"gates_{name}.json"), "w") as f:
            json.dump(rows, f)
    return res


# ------------------------------------------------------------------------- C5 --
def rel_motion(A, B):
    return pose_error(B, A)   # (degrees, mm) of A^-1 B


def track_rgbd(fr, rgb):
    """The trajectory of the sequence tracked with colour, frame 0 the origin."""
    n = len(fr)
    traj = [np.eye(4)]
    with youth_rgbd.RgbdContext(W, H, 100) as ctx:
        for s in range(0, n - 1, 100):
            T_rel, st = ctx.track_host_sequence(fr[s:s + 101], rgb[s:s + 101])
            T_rel[:, 3, :] = (0.0, 0.0, 0.0, 1.0)
            for T in T_rel:
                traj.append(traj[-1] @ T)
    return np.array(traj)


def track_rgbd_streamed(fr, rgb, track_levels):
    """The same through the streaming tracker (b = 8, two submissions in flight)
    with its own level schedule (youth_rgbd_track_set_levels)."""
    n = len(fr)
    traj = []
    with youth_rgbd.RgbdContext(W, H, 16) as ctx:
        ctx.track_set_batch(8)
        ctx.track_set_levels(track_levels)
        sizes = []

        def collect():
            for _ in range(sizes.pop(0)):
                T, has, _ = ctx.track_collect()
                traj.append(traj[-1] @ T if has else np.eye(4))

        for s in range(0, n, 8):
            if len(sizes) == 2:
                collect()
            ctx.track_submit(list(fr[s:s + 8]), list(rgb[s:s + 8]))
            sizes.append(len(fr[s:s + 8]))
        while sizes:
            collect()
    return np.array(traj)


C5_FRAMES = (150, 200, 627, 800, 999)


def c5track(track_levels, n=1000):
    """C5's RGB-D tracking errors alone, without and with the tracker's schedule."""
    fr, X, rgb = youth_synth.sequence_rgb(0, n, W, H)
    gt = np.array([np.linalg.inv(X[0]) @ X[k] for k in range(n)])
    out = {}
    for name, lv in (("none", None), ("track_levels", track_levels)):
        t0 = time.perf_counter()
        T = track_rgbd_streamed(fr, rgb, lv)
        dt = time.perf_counter() - t0
        out[name] = {"levels": [list(l) for l in lv or ()], "frames_per_s": round(n / dt, 1)}
        for f in C5_FRAMES:
            if f < n:
                out[name][f"frame_{f}_deg_mm"] = [round(v, 4) for v in pose_error(T[f], gt[f])]
                if f >= 100:   # against the track from frame 100: the motion since then alone
                    out[name][f"frame_{f}_since_100_deg_mm"] = [round(v, 4) for v in pose_error(
                        np.linalg.inv(T[100]) @ T[f], np.linalg.inv(gt[100]) @ gt[f])]
        print(f"C5 tracking, tracker schedule {name}: {out[name]}", flush=True)
    return out


def close_trajectory(fr, rgb, T, levels=None):
    """Keyframes as the drop-in picks them, stored and closed in order, the pose
    graph optimised and the trajectory re-hung: (keyframes, loop edges, close ms
    per keyframe, optimise ms, cost before and after, corrected trajectory)."""
    n = len(fr)
    kf = [0]
    for f in range(1, n):
        deg, mm = rel_motion(T[kf[-1]], T[f])
        if mm > 100.0 or deg > 10.0:
            kf.append(f)
    kf = kf[:youth_loop.MAX_KEYFRAMES]
    t_close = []
    with youth_loop.LoopCloser(W, H, max(2, len(kf))) as lc:
        lc.set_levels(levels)
        for i, f in enumerate(kf):
            lc.add_keyframe(fr[f], rgb[f], T[f], tag=f)
            t0 = time.perf_counter()
            lc.close(i)
            t_close.append((time.perf_counter() - t0) * 1e3)
        loops = lc.edges()
    odo = [(i - 1, i, np.linalg.inv(T[kf[i - 1]]) @ T[kf[i]], 1.0) for i in range(1, len(kf))]
    edges = np.concatenate([youth_loop.make_edges(odo), loops])
    t0 = time.perf_counter()
    Xo, c0, c1 = youth_loop.optimize_pose_graph(T[kf], edges)
    t_opt = (time.perf_counter() - t0) * 1e3
    return kf, loops, t_close, t_opt, (c0, c1), youth_loop.interpolate(T, kf, T[kf], Xo)


def c5(n=1000, levels=None, track_levels=None):
    fr, X, rgb = youth_synth.sequence_rgb(0, n, W, H)
    gt = np.array([np.linalg.inv(X[0]) @ X[k] for k in range(n)])
    trajs = {}
    with youth_icp.IcpContext(W, H, 16) as ctx:
        ctx.track_set_batch(8)
        T_rel, st = ctx.track_host_sequence(fr)
        T_rel = T_rel[-(n - 1):]
    traj = [np.eye(4)]
    for k in range(n - 1):
        traj.append(traj[-1] @ T_rel[k])
    trajs["depth"] = np.array(traj)
    trajs["rgbd"] = track_rgbd(fr, rgb)
    if track_levels:
        trajs["rgbd+track_levels"] = track_rgbd_streamed(fr, rgb, track_levels)
    out = {}
    runs = [(name, T, None) for name, T in trajs.items()]
    if levels:
        runs += [(name + "+levels", T, levels) for name, T in trajs.items()]
    for name, T, lv in runs:
        kf, loops, t_close, t_opt, (c0, c1), closed = close_trajectory(fr, rgb, T, lv)
        edge_err = [pose_error(e["Z"], np.linalg.inv(gt[kf[e["i"]]]) @ gt[kf[e["j"]]]) for e in loops]
        res = {"keyframes": len(kf), "loop_edges": int(loops.shape[0]),
               "loop_edge_error_max_deg_mm": [round(max(e[0] for e in edge_err), 4),
                                              round(max(e[1] for e in edge_err), 3)] if edge_err else None,
               "close_ms_per_keyframe": stats(t_close), "optimize_ms": round(t_opt, 2),
               "cost": [c0, c1]}
        for f in C5_FRAMES:
            if f < n:
                res[f"frame_{f}_before_deg_mm"] = [round(v, 4) for v in pose_error(T[f], gt[f])]
                res[f"frame_{f}_after_deg_mm"] = [round(v, 4) for v in pose_error(closed[f], gt[f])]
        print(f"C5, {name} tracking: {res}", flush=True)
        if DUMP:
            with open(os.path.join(DUMP, f"c5_{name}.json"), "w") as f:
                json.dump({"kf": kf, "edges": [[int(e["i"]), int(e["j"]), *err, float(e["overlap"]),
                                                float(e["gray_rms"]), float(e["fb_rot_deg"]),
                                                float(e["fb_trans_m"]) * 1e3]
                                               for e, err in zip(loops, edge_err)],
                           "before": [pose_error(T[f], gt[f]) for f in range(0, n, 10)],
                           "after": [pose_error(closed[f], gt[f]) for f in range(0, n, 10)]}, f)
        out[name] = res
    return out


# ---------------------------------------------------------------------- C5 map --
MAP_VPM, MAP_SLOTS, MAP_CHUNK = 100.0, 1 << 25, 64


def c5map(n=1000):
    fr, X, rgb = youth_synth.sequence_rgb(0, n, W, H)
    gt = np.array([np.linalg.inv(X[0]) @ X[k] for k in range(n)])
    T = track_rgbd(fr, rgb)
    kf, loops, _, _, _, closed = close_trajectory(fr, rgb, T)
    # the frames on the device in chunks of 64, as the drop-in's store keeps them
    chunks = []
    for c0 in range(0, n, MAP_CHUNK):
        c1 = min(n, c0 + MAP_CHUNK)
        chunks.append((c0, c1, torch.from_numpy(np.stack(fr[c0:c1])).cuda(),
                       torch.from_numpy(np.stack(rgb[c0:c1])).cuda()))

    def poses(P):
        return [torch.from_numpy(np.ascontiguousarray(P[c0:c1].reshape(-1, 16)[:, :12], np.float32)).cuda()
                for c0, c1, _, _ in chunks]

    def keys(rec):
        return ((rec["iz"].astype(np.int64) + (1 << 20)) << 42) | \
               ((rec["iy"].astype(np.int64) + (1 << 20)) << 21) | (rec["ix"].astype(np.int64) + (1 << 20))

    def jaccard(a, b):
        both = np.intersect1d(a, b, assume_unique=True).shape[0]
        return both / max(1, a.shape[0] + b.shape[0] - both)

    P_gt, P_live, P_closed = poses(gt), poses(T), poses(closed)
    torch.cuda.synchronize()
    with youth_map.VoxelMap(MAP_VPM, MAP_SLOTS) as m:
        for (c0, c1, d, c), P in zip(chunks, P_gt):
            m.integrate_device(d.data_ptr(), c.data_ptr(), c1 - c0, W, H, P.data_ptr())
        k_gt = keys(m.extract())
        dropped = m.stats()["dropped"]
        m.clear()
        for (c0, c1, d, c), P in zip(chunks, P_live):
            m.integrate_device(d.data_ptr(), c.data_ptr(), c1 - c0, W, H, P.data_ptr())
        k_live = keys(m.extract())
        m.sync()
        t0 = time.perf_counter()
        for (c0, c1, d, c), P0, P1 in zip(chunks, P_live, P_closed):
            m.move_device(d.data_ptr(), c.data_ptr(), c1 - c0, W, H, P0.data_ptr(), P1.data_ptr())
        m.sync()
        t_move = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        m.compact()
        t_compact = (time.perf_counter() - t0) * 1e3
        k_closed = keys(m.extract())
        st, rs = m.stats(), m.remove_stats()
    moved = int(sum(not np.array_equal(a.reshape(-1)[:12].astype(np.float32),
                                       b.reshape(-1)[:12].astype(np.float32)) for a, b in zip(T, closed)))
    res = {"frames": n, "vpm": MAP_VPM, "slots": MAP_SLOTS, "keyframes": len(kf),
           "loop_edges": int(loops.shape[0]), "frames_moved": moved,
           "voxels_gt": int(k_gt.shape[0]), "voxels_before": int(k_live.shape[0]),
           "voxels_after": int(k_closed.shape[0]),
           "jaccard_before": round(jaccard(k_live, k_gt), 4),
           "jaccard_after": round(jaccard(k_closed, k_gt), 4),
           "reintegrate_ms": round(t_move, 2), "reintegrate_us_per_moved_frame": round(t_move * 1e3 / max(1, moved), 1),
           "compact_ms": round(t_compact, 2),
           "dropped": int(dropped + st["dropped"]), "missing": rs["missing"], "underflow": rs["underflow"],
           "stale": rs["stale"]}
    print(f"C5 map, rgbd tracking: {res}", flush=True)
    return res


DUMP = None   # dump=DIR: every verified pair and every loop edge as JSON files there


def main():
    global DUMP
    args = sys.argv[1:]
    levels = None
    if "--levels" in args:
        k = args.index("--levels")
        levels = youth_rgbd.parse_levels(args[k + 1], W, H)
        del args[k:k + 2]
    track_levels = None
    if "--track-levels" in args:
        k = args.index("--track-levels")
        track_levels = youth_rgbd.parse_levels(args[k + 1], W, H)
        del args[k:k + 2]
    for a in args:
        if a.startswith("dump="):
            DUMP = a[5:]
            os.makedirs(DUMP, exist_ok=True)
    parts = [a for a in args if not a.startswith("dump=")] or ["kernels", "gates", "c5"]
    res = {"size": [W, H], "params": youth_loop.default_params().as_dict()}
    if "kernels" in parts:
        res["kernels"] = kernel_times()
    if levels:
        res["levels"] = [list(l) for l in levels]
    if "gates" in parts:
        def both(lv, tag):
            return {"default_noise": gate_table(youth_synth.DEFAULT_FLAGS, "DEFAULT_FLAGS" + tag, levels=lv),
                    "survey_noise": gate_table(youth_synth.SURVEY_FLAGS, "SURVEY_FLAGS" + tag, levels=lv)}
        res["gates"] = {"none": both(None, ""), "levels": both(levels, "_levels")} if levels else both(None, "")
    if "c5" in parts:
        res["c5"] = c5(levels=levels, track_levels=track_levels)
    if "c5track" in parts:
        res["c5track"] = c5track(track_levels or youth_rgbd.default_levels(W, H))
    if "c5map" in parts:
        res["c5map"] = c5map()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
