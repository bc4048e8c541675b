#!/usr/bin/env python3
"""The RGB-D alignment (kernels csrc/rgbd_align.hip, host csrc/rgbd_api.cpp;
DESIGN.md §13) by the numbers, run
by hand (not part of bench.py).  One process, HIP events, the variants
alternating within every round:

  (1) rate      time per align of youth_rgbd_align_pairs_device against
                youth_icp_align_pairs_device on its per-iteration path
                (YOUTH_ICP_NO_PERSISTENT=1 with YOUTH_ICP_NO_COOP=1, the
                like-for-like launch structure) and on its default plan, at 1,
                16 and 512 pairs of 640x480;
                the RGB-D align's 23 B per pixel and iteration as a fraction of
                8 TB/s, for the whole align (preps included) and for one
                k_rgbd_reduce launch (the align less the same align with no
                iterations, over the iterations); k_rgbd_prep per frame
  (2) accuracy  pairs 0->1, 1->2, 3->4, 5->6 and the composed pose at frames 7,
                16 and 31 of the 640x480 synthetic sequence against T_wc, for
                lambda = 0 and 0.1, at the default noise, at SURVEY §8d noise
                raw and at SURVEY §8d noise with every frame through
                youth_depth_filter_device

With --levels SPEC (`auto`, or stride:iterations items such as 8:10,1:10;
DESIGN.md §16) part (1) also times the same align on a context with that level
schedule (rgbd_levels) and k_rgbd_decimate alone at the schedule's first
stride (per frame; a scheduled pair call decimates two frames per pair), in
the same rounds, and part (2) is left out.

The last line is one JSON object.
usage: python tools/rgbd_bench.py [rounds] [reps] [--levels SPEC]"""
import json
import os
import sys

import torch  # noqa: F401  (first: shared HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-rgbd_amd"))
import numpy as np  # noqa: E402

import youth_filter  # noqa: E402
import youth_icp  # noqa: E402
import youth_rgbd  # noqa: E402
import youth_synth  # noqa: E402

W, H = 640, 480
HBM_BYTES_PER_S = 8e12
BYTES_PER_PX_ITER = 23      # depth 2 + Y 1 + record 16 + word 4


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3),
            "max": round(float(np.max(v)), 3)}


def rate(rounds, reps, levels=None):
    src, dst, _, srgb, drgb = youth_synth.pairs_rgb(0, 8, W, H)
    sg, dg = youth_synth.luma(srgb), youth_synth.luma(drgb)
    s = torch.cuda.Stream()
    out = {}
    for n in (1, 16, 512):
        pick = np.arange(n) % 8
        d = [torch.from_numpy(np.ascontiguousarray(a[pick])).cuda() for a in (src, sg, dst, dg)]
        torch.cuda.synchronize()
        rgbd = youth_rgbd.RgbdContext(W, H, max(n, 2))
        rgbd0 = youth_rgbd.RgbdContext(W, H, max(n, 2), iters=0)    # the preps and k_init alone
        # NO_COOP too: a small batch would otherwise take the cooperative kernel first
        os.environ["YOUTH_ICP_NO_PERSISTENT"] = os.environ["YOUTH_ICP_NO_COOP"] = "1"
        icp_iter = youth_icp.IcpContext(W, H, max(n, 2))
        del os.environ["YOUTH_ICP_NO_PERSISTENT"], os.environ["YOUTH_ICP_NO_COOP"]
        icp = youth_icp.IcpContext(W, H, max(n, 2))
        run = {
            "rgbd": lambda: rgbd.align_pairs_device(d[0], d[1], d[2], d[3], n, stream=s.cuda_stream),
            "rgbd_no_iterations": lambda: rgbd0.align_pairs_device(d[0], d[1], d[2], d[3], n,
                                                                   stream=s.cuda_stream),
            "icp_per_iteration": lambda: icp_iter.align_pairs_device(
                d[0].data_ptr(), d[2].data_ptr(), n, stream=s.cuda_stream),
            "icp_default": lambda: icp.align_pairs_device(d[0].data_ptr(), d[2].data_ptr(), n,
                                                          stream=s.cuda_stream),
            "rgbd_prep": lambda: rgbd.prep_device(d[3], 1, n, None, words, stream=s.cuda_stream),
        }
        words = torch.empty((n, H * W), dtype=torch.int32, device="cuda")
        ctxs = [rgbd, rgbd0, icp_iter, icp]
        if levels:
            rgbd_lv = youth_rgbd.RgbdContext(W, H, max(n, 2))
            rgbd_lv.set_levels(levels)
            ctxs.append(rgbd_lv)
            s0 = levels[0][0]
            lo = [torch.empty((n, (H + s0 - 1) // s0, (W + s0 - 1) // s0), dtype=dt, device="cuda")
                  for dt in (torch.int16, torch.uint8)]
            run["rgbd_levels"] = lambda: rgbd_lv.align_pairs_device(d[0], d[1], d[2], d[3], n,
                                                                    stream=s.cuda_stream)
            if s0 > 1:
                run["decimate"] = lambda: youth_rgbd.decimate_device(
                    d[0].data_ptr(), d[1].data_ptr(), n, W, H, s0, lo[0].data_ptr(), lo[1].data_ptr(),
                    stream=s.cuda_stream)
        calls = max(1, 32 // n)
        t = {k: [] for k in run}
        for r in range(rounds + 1):                    # round 0 warms up
            for _ in range(reps):
                for name, fn in run.items():
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    for _ in range(calls):
                        fn()
                    e1.record(s)
                    e1.synchronize()
                    if r > 0:
                        t[name].append(e0.elapsed_time(e1) / (calls * n) * 1e3)
        res = {k: stats(v) for k, v in t.items()}      # us per align (per frame for the prep)
        us = res["rgbd"]["median"]
        res["plans"] = {"icp_per_iteration": icp_iter.get_plan()["kernel"],
                        "icp_default": icp.get_plan()["kernel"]}
        res["rgbd_over_icp_per_iteration"] = round(us / res["icp_per_iteration"]["median"], 3)
        res["rgbd_over_icp_default"] = round(us / res["icp_default"]["median"], 3)
        res["rgbd_fraction_of_8TBs"] = round(
            BYTES_PER_PX_ITER * W * H * rgbd.iters / (us * 1e-6) / HBM_BYTES_PER_S, 4)
        # one k_rgbd_reduce launch per pair: the align less the same align without iterations
        k_us = (us - res["rgbd_no_iterations"]["median"]) / rgbd.iters
        res["k_rgbd_reduce_us_per_pair"] = round(k_us, 3)
        res["k_rgbd_reduce_fraction_of_8TBs"] = round(
            BYTES_PER_PX_ITER * W * H / (k_us * 1e-6) / HBM_BYTES_PER_S, 4)
        if levels:
            res["levels"] = [list(l) for l in levels]
            res["rgbd_levels_over_rgbd"] = round(res["rgbd_levels"]["median"] / us, 3)
        out[str(n)] = res
        print(f"{n:4d} pairs: {res}", flush=True)
        for c in ctxs:
            c.close()
        del d, words, run
    return out


def accuracy():
    n = 32
    out = {}
    for noise, flags, filt in (("default", youth_synth.DEFAULT_FLAGS, False),
                               ("survey_raw", youth_synth.SURVEY_FLAGS, False),
                               ("survey_filtered", youth_synth.SURVEY_FLAGS, True)):
        fr, Twc, rgb = youth_synth.sequence_rgb(0, n, W, H, flags=flags)
        d_depth = torch.from_numpy(fr).cuda()
        if filt:
            d_depth = youth_filter.depth_filter_device(d_depth)
        d_gray = youth_rgbd.luma_device(torch.from_numpy(rgb).cuda())
        torch.cuda.synchronize()
        for lam in (0.0, 0.1):
            with youth_rgbd.RgbdContext(W, H, n - 1, lam=lam) as ctx:
                ctx.align_sequence_device(d_depth, d_gray, n)
                T, _, st = ctx.poses(n - 1)
            res = {"status_or": int(np.bitwise_or.reduce(st))}
            for k in (0, 1, 3, 5):
                e = pose_error(T[k], np.linalg.inv(Twc[k]) @ Twc[k + 1])
                res[f"pair_{k}_{k + 1}"] = [round(e[0], 4), round(e[1], 3)]
            C = np.eye(4)
            for k in range(n - 1):
                C = C @ T[k]
                if k + 1 in (7, 16, 31):
                    e = pose_error(C, np.linalg.inv(Twc[0]) @ Twc[k + 1])
                    res[f"frame_{k + 1}"] = [round(e[0], 4), round(e[1], 3)]
            out[f"{noise}_lambda_{lam}"] = res
            print(f"{noise:16s} lambda {lam}: {res}  (deg, mm)", flush=True)
    return out


def pose_error(T, T_gt):
    D = np.linalg.inv(T_gt) @ T
    ang = np.degrees(np.arccos(np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))
    return float(ang), float(np.linalg.norm(D[:3, 3]) * 1000.0)


def main():
    args = sys.argv[1:]
    levels = None
    if "--levels" in args:
        k = args.index("--levels")
        levels = youth_rgbd.parse_levels(args[k + 1], W, H)
        del args[k:k + 2]
    rounds = int(args[0]) if len(args) > 0 else 3
    reps = int(args[1]) if len(args) > 1 else 3
    res = {"size": [W, H], "params": list(youth_rgbd.default_params()),
           "us_per_align": rate(rounds, reps, levels)}
    if not levels:
        res["accuracy_deg_mm"] = accuracy()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
