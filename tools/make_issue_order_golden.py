#!/usr/bin/env python3
"""Write the fixtures of tests/test_gpu_issue_order.py: poses, statuses and
per-iteration match counts and r2 of every case of that file, as the library
in the tree computes them on the GPU.

Run it on the commit whose results are to be pinned, BEFORE the change under
test, never on the change itself:

    python3 tools/make_issue_order_golden.py [out_dir]

out_dir defaults to tests/golden/issue_order.  Every case runs twice and must
repeat bit for bit before it is written.  The cases, shapes and seeds are the
test file's own (CASES, run_case), so fixture and test cannot drift apart.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("slam-rgbd_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import torch  # noqa: E402,F401  (first: the HIP runtime the library binds to)
import numpy as np  # noqa: E402

import test_gpu_issue_order as t  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN_DIR
    os.makedirs(out, exist_ok=True)
    total = 0
    for name in sorted(t.CASES):
        a, b = t.run_case(name), t.run_case(name)
        for f in t.FIELDS:
            if a[f].tobytes() != b[f].tobytes():
                raise SystemExit(f"{name}: {f} does not repeat bit for bit; nothing to pin")
        if a["first"] != "prep" or "k_icp (persistent)" not in a["plan"]:
            raise SystemExit(f"{name}: ran {a['first']} / {a['plan']}, not k_prep_ident + k_icp")
        path = os.path.join(out, name + ".npz")
        np.savez_compressed(path, **{f: a[f] for f in t.FIELDS})
        total += os.path.getsize(path)
        print(f"{name:32s} st {int(np.abs(a['st']).max())} cnt min {int(a['cnt'].min()):6d} "
              f"sched (polls, waited) {a['sched']}  {os.path.getsize(path)} B", flush=True)
    print(f"{len(t.CASES)} fixtures, {total} bytes -> {out}")


if __name__ == "__main__":
    main()
