"""Every launch plan of k_icp_coop and k_icp against the oracle.

The rest of the GPU suite runs the launch geometries a 256-CU device's planner
picks for its shapes.  Both align kernels take their geometry as launch
parameters, and a device with another CU count (a partitioned MI355X) picks
other values by itself, so this module forces them through the documented
environment knobs (DESIGN.md §6 "Knobs") and holds every plan to the same
results:

  * k_icp_coop at every pixels-per-lane count 1..32 (the groups-of-4 loop with
    each tail, the tail-0 case included), in its 512- and its 256-thread
    instantiations, with contiguous and with tile-shaped source chunks whose
    tiles are ragged at the right and bottom edges, and the 64x80-tile kernel;
  * the tracker's micro-batches on those plans (YOUTH_ICP_PULL_RESERVE_CU);
  * k_icp with 1..8 work queues, fewer pairs than queues, pair counts that no
    queue count divides, and set_concurrency 1..4;
  * reduce_geometry under YOUTH_ICP_TARGET_CHUNKS (one chunk per pair, the
    max_nb clamp);
  * k_pull_frames with 1, 3 and 1024 workgroups per frame on frames of
    N % 8 == 0, odd N and N % 8 == 4.

Every plan: status 0 and equal to the oracle's (no TIMEOUT), per-iteration
correspondence counts equal to the oracle's, sum r^2 within rel 1e-6, fp64
poses within SAME_VARIANT_TOL of the oracle in the same reduction AND of the
default plan's pose of the same pair (the README's launch-independence claim
across plans), the fp32 device output equal to T32 bit for bit, and
get_plan() / lanes() reporting the forced geometry, so that no case passes by
running the default plan.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
import youth_icp
import youth_synth
from conftest import ORACLE, PKG, lanes_of, oracle_like

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-5            # test_gpu_reduce.POSE_TOL: lane32 poses vs the exact oracle
# test_gpu_reduce.SAME_VARIANT_TOL: poses vs the oracle in the same reduction,
# and here also an exact-reduction pose vs the default plan's pose of the same
# pair (fp64 summation order only).  Largest observed over every plan of this
# module: 3.95e-14 between plans, 9.04e-13 against the oracle (HISTORY.md,
# "Launch plans under test").
SAME_VARIANT_TOL = 1e-9
ITERS = 10
PERSISTENT = "k_prep + k_icp (persistent)"
KNOBS = ("YOUTH_ICP_COOP_PX", "YOUTH_ICP_COOP_THREADS", "YOUTH_ICP_COOP_TILE_SRC",
         "YOUTH_ICP_NO_COOP", "YOUTH_ICP_QUEUES", "YOUTH_ICP_TARGET_CHUNKS",
         "YOUTH_ICP_PULL_WG", "YOUTH_ICP_PULL_RESERVE_CU", "YOUTH_ICP_TRACK_COPY")

_observed = {"cross_plan": 0.0, "oracle": 0.0}


def _err(a, b):
    return float(np.abs(np.asarray(a)[..., :3, :4] - np.asarray(b)[..., :3, :4]).max())


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _inputs(W, H, n=11):
    """youth_synth.pairs(40, n, W, H) (pair p does not depend on n) and the
    initial poses: identity, but pair 2 starts 1 degree and 1 cm off."""
    src, dst, _ = youth_synth.pairs(40, n, W, H)
    T_init = np.tile(np.eye(4), (n, 1, 1))
    T_init[2] = oracle.se3_exp(np.r_[0.0, np.deg2rad(1.0), 0.0, 0.01, 0.0, 0.0])
    return _frozen(src, dst, T_init)


@functools.lru_cache(maxsize=None)
def _oracle_pair(W, H, p, lanes=None):
    """(T64, status, counts [ITERS], sum r^2 [ITERS]) of pair p from the CPU
    oracle: EXACT (lanes None), or LANE32 over the partition `lanes`."""
    src, dst, T_init = _inputs(W, H)
    with oracle_like(lanes):
        T64, _, st, stats = oracle.align(src[p], dst[p], iters=ITERS, T_init=T_init[p])
    T64, cnt, r2 = _frozen(T64, stats[:, 0].copy(), stats[:, 1].copy())
    return T64, int(st), cnt, r2


def _device_inputs(W, H, n):
    src, dst, T_init = _inputs(W, H)
    ds, dd = torch.from_numpy(src[:n].copy()).cuda(), torch.from_numpy(dst[:n].copy()).cuda()
    out = torch.zeros((n, 16), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return ds, dd, out, T_init[:n]


def _align_twice(ctx, dev, n):
    """Two aligns on the same context (the arena and counter-set alternation
    run under the forced geometry); the second one's results."""
    ds, dd, out, T_init = dev
    out.zero_()
    for _ in range(2):
        ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), n, T_init=T_init,
                               d_T_out=out.data_ptr())
    ctx.sync()
    T64, T32, st = ctx.get_poses(n)
    cnt, r2 = ctx.get_stats(n, ITERS)
    return {"T64": T64, "T32": T32, "st": st, "cnt": cnt, "r2": r2, "plan": ctx.get_plan(),
            "lanes": ctx.lanes(), "Tdev": out.cpu().numpy().reshape(n, 4, 4)}


@functools.lru_cache(maxsize=None)
def _default_plan_poses(W, H):
    """fp64 poses of the first 3 pairs on the plan the library picks by
    itself, EXACT reduction.  Called before a test sets any knob."""
    assert not [k for k in KNOBS if k in os.environ], "a plan knob is already set"
    dev = _device_inputs(W, H, 3)
    with youth_icp.IcpContext(W, H, 3, iters=ITERS) as ctx:
        res = _align_twice(ctx, dev, 3)
    return _frozen(res["T64"])[0]


def _check(res, W, H, n, what, red="exact", default=None, vs_exact=False):
    """The assertions every plan is held to (module docstring).  A lane32 pose
    is held to its own oracle; its distance from the EXACT oracle is the fp32
    rounding of the lane sums, a property of the reduction and the data that
    the CPU oracle shows alone (pair 2 of 120x150 over 64x80 tiles: 1.34e-5),
    so only vs_exact (160x120, test_coop_px_sweep_lane32) bounds it."""
    lanes = res["lanes"] if red == "lane32" else None
    for p in range(n):
        To, sto, cnt_o, r2_o = _oracle_pair(W, H, p, lanes)
        tag = (what, red, p)
        assert res["st"][p] == sto == 0, (tag, int(res["st"][p]), sto)
        assert np.array_equal(res["cnt"][p], cnt_o), (tag, res["cnt"][p], cnt_o)
        np.testing.assert_allclose(res["r2"][p], r2_o, rtol=1e-6, err_msg=str(tag))
        e = _err(res["T64"][p], To)
        _observed["oracle"] = max(_observed["oracle"], e)
        assert e <= SAME_VARIANT_TOL, (tag, e)
        if red == "lane32":
            if vs_exact:
                e = _err(res["T64"][p], _oracle_pair(W, H, p)[0])
                assert e <= POSE_TOL, (tag, e)
        elif default is not None and p < len(default):
            e = _err(res["T64"][p], default[p])
            _observed["cross_plan"] = max(_observed["cross_plan"], e)
            assert e <= SAME_VARIANT_TOL, (tag, e)
        assert np.array_equal(res["Tdev"][p], res["T32"][p]), tag


def _report(name):
    print(f"\n[plans] {name}: max |pose - default plan| {_observed['cross_plan']:.3e}, "
          f"max |pose - oracle| {_observed['oracle']:.3e} (bound {SAME_VARIANT_TOL:.0e})")


def _coop_kind(W, H, threads, npx):
    """launch_coop's rule: tile-shaped source chunks when one target tile (64 x
    24, or 64 x 80 for 512 threads) is exactly a workgroup's npx threads
    pixels and the pair has one workgroup per tile."""
    G = -(-W * H // (npx * threads))
    for th in (80, 24) if threads == 512 else (24,):
        if npx * threads == 64 * th and G == -(-W // 64) * -(-H // th):
            return youth_icp.LANES_COOP_TILE
    return youth_icp.LANES_COOP


def _expect_coop(res, W, H, threads, npx, kind, what):
    G = -(-W * H // (npx * threads))
    assert res["plan"] == {"kernel": "k_icp_coop", "workgroups_per_pair": G, "threads": threads,
                           "px_per_lane": npx}, (what, res["plan"])
    assert res["lanes"] == (kind, npx * threads, threads, npx), (what, res["lanes"])


# ------------------------------------------------------------ 1: coop px sweep --
COOP_REQUIRED_PX = {512: 22, 256: 32}   # the cooperative kernel MUST run up to here


@pytest.mark.parametrize("W,H", [(160, 120), (97, 53)])
@pytest.mark.parametrize("threads", [512, 256])
def test_coop_px_sweep(monkeypatch, threads, W, H):
    """k_icp_coop at every YOUTH_ICP_COOP_PX 1..32 (the pixel loop's groups of
    4 with tails 0..3, one to eight groups), 3 pairs, EXACT reduction, in the
    512- and the 256-thread instantiations.  160x120 (W % 4 == 0: the wide
    fused prep) runs G = 38..2 workgroups per pair at 512 threads with a
    ragged last chunk, 97x53 (the narrow prep) G = 11..1.  The cooperative
    kernel must take npx 1..22 at 512 threads (3 npx 512 4 B of dynamic LDS
    beside ~26.7 KB static fit 160 KB) and 1..32 at 256; above 22 at 512
    threads the occupancy query may find no fit, and then the persistent
    fallback is checked the same way."""
    n = 3
    default = _default_plan_poses(W, H)
    dev = _device_inputs(W, H, n)
    monkeypatch.setenv("YOUTH_ICP_COOP_THREADS", str(threads))
    admitted_above = []
    for npx in range(1, 33):
        monkeypatch.setenv("YOUTH_ICP_COOP_PX", str(npx))
        with youth_icp.IcpContext(W, H, n, iters=ITERS) as ctx:
            res = _align_twice(ctx, dev, n)
        what = (threads, W, H, npx)
        if npx <= COOP_REQUIRED_PX[threads] or res["plan"]["kernel"] == "k_icp_coop":
            # contiguous chunks, but 97x53 at 10 px x 512 is one 64x80 tile per workgroup
            _expect_coop(res, W, H, threads, npx, _coop_kind(W, H, threads, npx), what)
            if npx > COOP_REQUIRED_PX[threads]:
                admitted_above.append(npx)
        else:
            assert res["plan"] == {"kernel": PERSISTENT}, (what, res["plan"])
            assert res["lanes"][0] == youth_icp.LANES_STRIDED, (what, res["lanes"])
        _check(res, W, H, n, what, default=default)
    print(f"\n[plans] coop px above {COOP_REQUIRED_PX[threads]} admitted at {threads} threads, "
          f"{W}x{H}: {admitted_above}")
    _report(f"coop_px_sweep[{threads}-{W}x{H}]")


# ---------------------------------------------------- 2: coop px sweep, lane32 --
@pytest.mark.parametrize("threads", [512, 256])
def test_coop_px_sweep_lane32(monkeypatch, threads):
    """The lane partition k_icp_coop reports (youth_icp_get_lanes) is the one
    it ran, in both instantiations: under the oracle's LANE32 restatement of
    (LANES_COOP, npx threads, threads, npx) the per-iteration counts are equal
    and the poses within 1e-9; a partition reported wrongly (512 lanes for a
    256-thread workgroup) moves the fp32 lane sums and fails this."""
    W, H, n = 160, 120, 3
    dev = _device_inputs(W, H, n)
    monkeypatch.setenv("YOUTH_ICP_COOP_THREADS", str(threads))
    for npx in (1, 2, 3, 4, 5, 8, 12, 16):
        monkeypatch.setenv("YOUTH_ICP_COOP_PX", str(npx))
        with youth_icp.IcpContext(W, H, n, iters=ITERS, reduction="lane32") as ctx:
            res = _align_twice(ctx, dev, n)
            assert lanes_of(ctx) == res["lanes"]
        _expect_coop(res, W, H, threads, npx, youth_icp.LANES_COOP, (threads, npx))
        _check(res, W, H, n, (threads, npx), red="lane32", vs_exact=True)
    _report(f"coop_px_sweep_lane32[{threads}]")


# --------------------------------------------------- 3: ragged tile sources --
TILE_CASES = {
    # id: (W, H, threads, px, tile height)
    "128x48-512x3": (128, 48, 512, 3, 24),     # full 64x24 tiles, G = 4
    "128x48-256x6": (128, 48, 256, 6, 24),     # the 256-thread tile mapping
    "120x48-512x3": (120, 48, 512, 3, 24),     # ragged right edge, wide prep
    "120x48-256x6": (120, 48, 256, 6, 24),
    "118x47-512x3": (118, 47, 512, 3, 24),     # ragged right and bottom, narrow prep
    "128x160-512x10": (128, 160, 512, 10, 80),  # tall kernel, full 64x80 tiles
    "120x150-512x10": (120, 150, 512, 10, 80),  # tall kernel, ragged both edges
    "128x160-512x3": (128, 160, 512, 3, 24),   # 64x24 tiles, G = 14, ragged bottom row
}


@pytest.mark.parametrize("case", sorted(TILE_CASES))
def test_coop_ragged_tile_sources(monkeypatch, case):
    """Tile-shaped source chunks (one 64 x 24 or 64 x 80 target tile per
    workgroup) on frames whose last tile column and row are ragged, so the
    `u < W && v < H` edge of the source staging is false for some lanes, in
    both reductions, against contiguous chunks (YOUTH_ICP_COOP_TILE_SRC=0) on
    the same plan.  Every case forces the px per lane at which a pair has one
    workgroup per tile."""
    W, H, threads, npx, th = TILE_CASES[case]
    n = 3
    tiles = -(-W // 64) * -(-H // th)
    assert -(-W * H // (npx * threads)) == tiles and npx * threads == 64 * th   # the case itself
    default = _default_plan_poses(W, H)
    dev = _device_inputs(W, H, n)
    monkeypatch.setenv("YOUTH_ICP_COOP_THREADS", str(threads))
    monkeypatch.setenv("YOUTH_ICP_COOP_PX", str(npx))
    for tile_src in ("1", "0"):
        monkeypatch.setenv("YOUTH_ICP_COOP_TILE_SRC", tile_src)
        kind = youth_icp.LANES_COOP_TILE if tile_src == "1" else youth_icp.LANES_COOP
        for red in ("exact", "lane32"):
            with youth_icp.IcpContext(W, H, n, iters=ITERS, reduction=red) as ctx:
                res = _align_twice(ctx, dev, n)
            what = (case, tile_src)
            _expect_coop(res, W, H, threads, npx, kind, what)
            if th == 80:
                assert res["lanes"][1] == 5120
            _check(res, W, H, n, what, red=red, default=default)
    _report(f"coop_ragged_tile_sources[{case}]")


# ------------------------------------------- 4: tracker micro-batches, forced --
@functools.lru_cache(maxsize=None)
def _sequence(first, n, W, H):
    """Frames and the oracle's (T64, status) of every consecutive pair."""
    frames, _ = youth_synth.sequence(first, n, W, H)
    T, st = [], []
    for k in range(1, n):
        T64, _, s, _ = oracle.align(frames[k], frames[k - 1], iters=ITERS)
        T.append(T64)
        st.append(s)
    return _frozen(frames, np.stack(T), np.array(st, np.int32))


@pytest.mark.parametrize("reserve", ["0", "32", "128"])
@pytest.mark.parametrize("threads", [512, 256])
def test_track_micro_batches_forced_plans(monkeypatch, threads, reserve):
    """The tracker's chained micro-batches of 2, 3 and 8 frames with the CUs
    kept free for k_pull_frames forced to none, the default and half the
    chip (YOUTH_ICP_PULL_RESERVE_CU: another px per lane for the same batch),
    on 512- and 256-thread workgroups: youth_icp.h's contract, every frame
    bit-identical to track_frame on the same context, and within 1e-9 of the
    oracle with equal status."""
    monkeypatch.setenv("YOUTH_ICP_COOP_THREADS", str(threads))
    monkeypatch.setenv("YOUTH_ICP_PULL_RESERVE_CU", reserve)
    for W, H in ((160, 120), (97, 53)):
        frames, To, sto = _sequence(3, 17, W, H)
        with youth_icp.IcpContext(W, H, 16, iters=ITERS) as ctx:
            for m in (2, 3, 8):
                what = (threads, reserve, W, H, m)
                ctx.track_set_batch(m)
                ctx.track_reset()
                chained = ctx.track_chained_frames()
                Tb, stb = ctx.track_host_sequence(frames)
                assert ctx.track_chained_frames() > chained, what
                plan = ctx.get_plan()
                assert plan["kernel"] == "k_icp_coop" and plan["threads"] == threads, (what, plan)
                assert ctx.lanes()[2:] == (threads, plan["px_per_lane"]), (what, ctx.lanes())
                ctx.track_reset()
                want = [ctx.track_frame(f) for f in frames]
                assert ctx.get_plan() == plan, what          # the same plan frame by frame
                assert not want[0][2] and all(w[2] for w in want[1:]), what
                assert np.array_equal(Tb, np.stack([w[0] for w in want[1:]])), what
                assert np.array_equal(stb, np.array([w[1] for w in want[1:]], np.int32)), what
                assert np.array_equal(stb, sto), (what, stb, sto)
                e = _err(Tb, To)
                _observed["oracle"] = max(_observed["oracle"], e)
                assert e <= SAME_VARIANT_TOL, (what, e)
            assert ctx.track_chained_frames() > 0
    _report(f"track_micro_batches_forced_plans[{threads}-{reserve}]")


# ------------------------------------------------ 5: persistent queue sweep --
@pytest.mark.parametrize("W,H", [(97, 53), (160, 120)])
def test_persistent_queue_sweep(monkeypatch, W, H):
    """k_icp with 1, 2, 3, 5, 7 and 8 work queues (YOUTH_ICP_QUEUES; the
    default is 1 below 128 pairs) on 1, 2, 5, 8 and 11 pairs: fewer pairs than
    queues (queues that hold no pair), as many, and pair counts the queue
    count does not divide; 97x53 has 3 chunks per pair, 160x120 has 10.  With
    1 and 8 queues also every set_concurrency share 1..4 (a smaller grid and
    fewer chunks)."""
    default = _default_plan_poses(W, H)
    monkeypatch.setenv("YOUTH_ICP_NO_COOP", "1")
    devs = {n: _device_inputs(W, H, n) for n in (1, 2, 5, 8, 11)}
    for nq in (1, 2, 3, 5, 7, 8):
        monkeypatch.setenv("YOUTH_ICP_QUEUES", str(nq))
        with youth_icp.IcpContext(W, H, 11, iters=ITERS) as ctx:
            for share in ((1, 2, 3, 4) if nq in (1, 8) else (1,)):
                ctx.set_concurrency(share)
                for n, dev in devs.items():
                    res = _align_twice(ctx, dev, n)
                    what = (W, H, nq, share, n)
                    assert res["plan"] == {"kernel": PERSISTENT}, (what, res["plan"])
                    kind, chunk, threads, _ = res["lanes"]
                    assert kind == youth_icp.LANES_STRIDED and threads == 256 and \
                        chunk % 1024 == 0, (what, res["lanes"])
                    ctx.get_sched_stats()
                    _check(res, W, H, n, what, default=default)
    _report(f"persistent_queue_sweep[{W}x{H}]")


# ---------------------------------------------------- 6: TARGET_CHUNKS knob --
_CHILD = r"""
import json, sys
import torch
import numpy as np
import oracle, youth_icp, youth_synth
W, H, n, iters = 160, 120, 5, 10
src, dst, _ = youth_synth.pairs(40, n, W, H)
T_init = np.tile(np.eye(4), (n, 1, 1))
T_init[2] = oracle.se3_exp(np.r_[0.0, np.deg2rad(1.0), 0.0, 0.01, 0.0, 0.0])
ds, dd = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
out = torch.zeros((n, 16), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
with youth_icp.IcpContext(W, H, n, iters=iters) as ctx:
    for _ in range(2):
        ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), n, T_init=T_init,
                               d_T_out=out.data_ptr())
    ctx.sync()
    T64, T32, st = ctx.get_poses(n)
    cnt, r2 = ctx.get_stats(n, iters)
    res = {"T64": T64.tolist(), "T32": T32.astype(np.float64).tolist(), "st": st.tolist(),
           "cnt": cnt.tolist(), "r2": r2.tolist(), "plan": ctx.get_plan(),
           "lanes": list(ctx.lanes()),
           "Tdev": out.cpu().numpy().astype(np.float64).reshape(n, 4, 4).tolist()}
print("RESULT " + json.dumps(res))
"""


def test_target_chunks_knob():
    """reduce_geometry under YOUTH_ICP_TARGET_CHUNKS, which the library reads
    once per process: one fresh child process per value aligns 5 pairs at
    160x120 on the persistent kernel.  "1": a single chunk per pair (chunk >=
    W H); "7": two chunks per pair; "1000000": the max_nb clamp (chunk ==
    2048, at least 8 pixels per lane)."""
    W, H, n = 160, 120, 5
    default = _default_plan_poses(W, H)
    env = dict(os.environ, YOUTH_ICP_NO_COOP="1",
               PYTHONPATH=os.pathsep.join([PKG, ORACLE] + [p for p in sys.path if p]))
    chunks = {}
    for value in ("1", "7", "1000000"):
        env["YOUTH_ICP_TARGET_CHUNKS"] = value
        r = subprocess.run([sys.executable, "-c", _CHILD], env=env, timeout=120,
                           capture_output=True, text=True)
        assert r.returncode == 0, (value, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        res = json.loads(line[len("RESULT "):])
        for k in ("T64", "cnt", "r2"):
            res[k] = np.array(res[k], np.float64)
        res["T32"] = np.array(res["T32"], np.float64).astype(np.float32)
        res["Tdev"] = np.array(res["Tdev"], np.float64).astype(np.float32)
        res["st"] = np.array(res["st"], np.int32)
        res["lanes"] = tuple(res["lanes"])
        assert res["plan"] == {"kernel": PERSISTENT}, (value, res["plan"])
        kind, chunk, threads, _ = res["lanes"]
        assert kind == youth_icp.LANES_STRIDED and threads == 256, (value, res["lanes"])
        chunks[value] = chunk
        _check(res, W, H, n, ("target_chunks", value), default=default)
    assert chunks["1"] >= W * H, chunks
    assert chunks["7"] == 10240, chunks       # ceil(7 / 5) = 2 chunks of ceil(19200 / 2) -> x 1024
    assert chunks["1000000"] == 2048, chunks
    _report("target_chunks_knob")


# ------------------------------------------------- 7: k_pull_frames grids --
_sdma_poses = {}


def _track_pinned(W, H, frames):
    """9 frames through track_submit_pinned in micro-batches of 4."""
    with youth_icp.IcpContext(W, H, 8, iters=ITERS) as ctx:
        ctx.track_set_batch(4)
        bufs = [youth_icp.PinnedFrame(H, W) for _ in frames]
        try:
            for b, f in zip(bufs, frames):
                b.array[:] = f
            T, st = [], []
            for i in range(0, len(bufs), 4):
                ctx.track_submit_pinned(bufs[i:i + 4])
                while ctx.track_pending():
                    Tk, s, has = ctx.track_collect()
                    if has:
                        T.append(Tk)
                        st.append(s)
            assert ctx.track_chained_frames() > 0
        finally:
            for b in bufs:
                b.close()
    return np.stack(T), np.array(st, np.int32)


@pytest.mark.parametrize("W,H", [(160, 120), (97, 53), (90, 50)])
@pytest.mark.parametrize("wg", ["1", "3", "1024"])
def test_pull_frames_grid_and_tails(monkeypatch, wg, W, H):
    """k_pull_frames with 1, 3 and 1024 workgroups per frame
    (YOUTH_ICP_PULL_WG): 1024 x 64 lanes outnumber a frame's 16-byte pieces,
    so only the vector tail loop runs.  160x120: the vector body; 97x53 (odd
    N): every frame but the first of a launch element by element; 90x50 (N %
    8 == 4): frame 0 the vector body plus the element tail, frame 1
    misaligned.  Poses bit-identical to the copy engine's
    (YOUTH_ICP_TRACK_COPY=sdma) and within 1e-9 of the oracle."""
    frames, To, sto = _sequence(17, 9, W, H)
    if (W, H) not in _sdma_poses:
        monkeypatch.setenv("YOUTH_ICP_TRACK_COPY", "sdma")
        _sdma_poses[W, H] = _frozen(*_track_pinned(W, H, frames))
        monkeypatch.delenv("YOUTH_ICP_TRACK_COPY")
    monkeypatch.setenv("YOUTH_ICP_PULL_WG", wg)
    T, st = _track_pinned(W, H, frames)
    Ts, sts = _sdma_poses[W, H]
    assert np.array_equal(T, Ts) and np.array_equal(st, sts), (wg, W, H)
    assert np.array_equal(st, sto), (wg, W, H, st, sto)
    e = _err(T, To)
    _observed["oracle"] = max(_observed["oracle"], e)
    assert e <= SAME_VARIANT_TOL, (wg, W, H, e)
    _report(f"pull_frames_grid_and_tails[{wg}-{W}x{H}]")
