"""Bit-for-bit pins of k_icp and k_prep_ident (icp_kernels.hip) across changes
that move no floating-point operation: wave priority around the projection
phase of k_icp's pixel loop (YOUTH_ICP_PRIO), and any edit of k_prep_ident's
row loop that touches only its addressing, its loads' form or its match count
(scalar row offsets with empty descriptors for rows outside the image and a
scalar match count were built against these pins; HISTORY.md).

The fixtures under tests/golden/issue_order/ were written by
tools/make_issue_order_golden.py on an MI355X from the commit BEFORE those
changes: poses (T64, T32), statuses and the per-iteration match counts and r2
of every case below.  A lane's pixel order, every fp32 expression and every
summation tree are what they were, so each case must reproduce its fixture
exactly, with the priority knob on, with it off (YOUTH_ICP_PRIO=0) and on a
repeat.  Everything runs on the persistent path (YOUTH_ICP_NO_COOP=1):
k_prep_ident (target records and iteration 0), then k_icp (iterations 1-9).

k_icp cases (both specs):
  97x53 x 3    W % 4 != 0: the unaligned pixel loop
  68x32 x 3    W % 4 == 0: the aligned pixel loop (depth prefetch)
  36x20 x 130  >= 128 pairs: eight work queues
  320x240 x 2  "items wait": two pairs in some 38 chunks each on a grid wider
               than the whole queue, so the items of the later iterations are
               claimed before their pair's pose exists and thread 0 polls the
               epoch (608 items waited on the parent commit).
               The test asserts items_waited > 0 with the knob off and on:
               a workgroup waits while others run at raised priority.
prep-form cases (the shapes of test_gpu_prep_columns.py): ragged columns
63x5, 65x9, 127x11; 66x50 in bands of 7 rows and of 1 row; 130x97 whose
second frame base is only 2-byte aligned; a 9-frame 65x9 sequence whose last
frame is no pair's target.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

import youth_icp
import youth_synth

pytestmark = pytest.mark.gpu
ITERS = 10
SEED = 50
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "issue_order")
FIELDS = ("T64", "T32", "st", "cnt", "r2")
KNOBS = ("YOUTH_ICP_NO_IDENT_FIRST", "YOUTH_ICP_IDENT_FIRST", "YOUTH_ICP_PREP_BAND",
         "YOUTH_ICP_QUEUES", "YOUTH_ICP_PRIO", "YOUTH_ICP_NO_PERSISTENT",
         "YOUTH_ICP_TARGET_CHUNKS", "YOUTH_ICP_SPEC", "YOUTH_ICP_REDUCE")

# name -> (W, H, frames, spec, band, sequence)
CASES = {}
for _spec in ("survey", "fma"):
    CASES[f"icp_unaligned_97x53_{_spec}"] = (97, 53, 3, _spec, None, False)
    CASES[f"icp_aligned_68x32_{_spec}"] = (68, 32, 3, _spec, None, False)
    CASES[f"icp_queues8_36x20_{_spec}"] = (36, 20, 130, _spec, None, False)
    CASES[f"prep_band7_66x50_{_spec}"] = (66, 50, 2, _spec, 7, False)
    CASES[f"prep_band1_66x50_{_spec}"] = (66, 50, 2, _spec, 1, False)
    CASES[f"prep_base2_130x97_{_spec}"] = (130, 97, 2, _spec, 16, False)
CASES["icp_items_wait_320x240"] = (320, 240, 2, "survey", None, False)
CASES["prep_ragged_63x5"] = (63, 5, 3, "survey", None, False)
CASES["prep_ragged_65x9"] = (65, 9, 3, "survey", None, False)
CASES["prep_ragged_127x11"] = (127, 11, 3, "survey", None, False)
CASES["prep_sequence_65x9"] = (65, 9, 9, "survey", None, True)
WAIT_CASE = "icp_items_wait_320x240"


@contextlib.contextmanager
def _env(**kv):
    """The knobs a context reads at creation: every one unset but `kv`."""
    old = {k: os.environ.get(k) for k in (*KNOBS, "YOUTH_ICP_NO_COOP")}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ["YOUTH_ICP_NO_COOP"] = "1"
    for k, v in kv.items():
        if v is not None:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_case(name, prio=None):
    """One device align of case `name` in a fresh context -> the FIELDS, the
    first iteration's form and the scheduler's (epoch polls, items waited)."""
    W, H, n, spec, band, sequence = CASES[name]
    if sequence:
        src, _ = youth_synth.sequence(SEED, n, W, H)
        dst = None
    else:
        src, dst, _ = youth_synth.pairs(SEED, n, W, H)
    with _env(YOUTH_ICP_PREP_BAND=band, YOUTH_ICP_PRIO=prio):
        ds = torch.from_numpy(src).cuda()
        dd = torch.from_numpy(dst).cuda() if dst is not None else None
        torch.cuda.synchronize()
        with youth_icp.IcpContext(W, H, max(n, 2), iters=ITERS, spec=spec) as ctx:
            if sequence:
                ctx.align_sequence_device(ds.data_ptr(), n)
                n -= 1
            else:
                ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), n)
            ctx.sync()
            T64, T32, st = ctx.get_poses(n)
            cnt, r2 = ctx.get_stats(n, ITERS)
            return {"T64": T64, "T32": T32, "st": st, "cnt": cnt, "r2": r2,
                    "first": ctx.get_first_iter(), "plan": ctx.get_plan()["kernel"],
                    "sched": ctx.get_sched_stats()}


def golden_path(name):
    return os.path.join(GOLDEN_DIR, name + ".npz")


def _same_bits(a, b, what):
    for f in FIELDS:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        assert x.dtype == y.dtype and x.shape == y.shape, (what, f, x.dtype, y.dtype, x.shape, y.shape)
        if x.tobytes() != y.tobytes():
            bad = np.argwhere(x.view(np.uint8).reshape(-1) != y.view(np.uint8).reshape(-1))
            raise AssertionError(f"{what}: {f} differs, first at byte {int(bad[0][0])} of {x.nbytes}")


@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_of_the_parent(name):
    """Knob default, a repeat, and knob off: each equals the parent's fixture
    bit for bit (so they also equal each other)."""
    gold = dict(np.load(golden_path(name)))
    on = run_case(name)
    again = run_case(name)
    off = run_case(name, prio=0)
    for r in (on, again, off):
        assert r["first"] == "prep" and "k_icp (persistent)" in r["plan"], (name, r["first"], r["plan"])
    # no case is vacuous: every pair converged on a real number of matches
    assert not gold["st"].any() and (gold["cnt"] >= 100).all(), (name, gold["st"], gold["cnt"].min())
    print(f"{name}: sched on {on['sched']} off {off['sched']}, cnt0 {on['cnt'][:3, 0]}")
    _same_bits(on, gold, f"{name}: knob default vs the parent")
    _same_bits(off, gold, f"{name}: knob off vs the parent")
    _same_bits(again, on, f"{name}: repeat")
    _same_bits(on, off, f"{name}: knob on vs off")
    if name == WAIT_CASE:
        # the shape's reason: items are claimed ahead of their pose
        assert off["sched"][1] > 0, off["sched"]
        assert on["sched"][1] > 0, on["sched"]
