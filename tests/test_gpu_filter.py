"""GPU tests of the edge-preserving depth filter (include/youth_filter.h,
DESIGN.md §11): k_depth_filter against the numpy restatement bit for bit on
both load paths, the argument checks, and the tracker family with the filter
on: oracle parity, the tracker's own invariants (batched = per-frame, realign,
pinned submission), the device API left alone, the SLAM.h drop-in through
YOUTH_ICP_DEPTH_FILTER, and the accuracy the filter is there for."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import oracle
import youth_filter
import youth_icp
import youth_synth
from conftest import GOLDEN, ORACLE, PKG
from filter_truth import filter_truth
from test_filter import KAT, KAT_FRAMES, hand_case, kat_frame, pose_error

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-5       # GPU pose against the C oracle (the project's bound)
CROSS_PATH_TOL = 1e-9   # two GPU paths that differ in fp64 summation order
CFG = os.path.join(GOLDEN, "astra_camera.yaml")
PARAMS = [(8, 96), (40, 1000), (1, 0)]


def _device(frames, t0, t2):
    d = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    out = youth_filter.depth_filter_device(d, None, t0, t2)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _both(frames, t0, t2):
    """The two entry points' outputs, checked against the restatement."""
    want = filter_truth(frames, t0, t2)
    got_d = _device(frames, t0, t2)
    got_h = youth_filter.depth_filter_host(frames, t0, t2)
    assert got_d.dtype == np.int16 and np.array_equal(got_d, want)
    assert got_h.dtype == np.int16 and np.array_equal(got_h, want)
    return want


def _pose_err(A, B):
    return float(np.abs(np.asarray(A)[:3, :4] - np.asarray(B)[:3, :4]).max())


# ------------------------------------------------------------ bit-exactness --

@pytest.mark.parametrize("t0,t2", PARAMS)
@pytest.mark.parametrize("name", sorted(KAT_FRAMES))
def test_filter_bit_exact_on_the_known_frames(name, t0, t2):
    """24x16 (one partial tile), 97x53 (ragged: the scalar path), 160x120
    (the vector path, 3 x 8 tiles), both noise levels."""
    src = kat_frame(name)
    want = _both(src, t0, t2)
    for n, p, crc, total, _, _ in KAT:
        if n == name and p == (t0, t2):
            assert zlib.crc32(want.tobytes()) == crc and int(want.astype(np.int64).sum()) == total
    if (t0, t2) == (1, 0):
        assert np.array_equal(want, src)
    # the other frame of the pair and the other noise level as well
    i, W, H, flags = KAT_FRAMES[name]
    other = youth_synth.DEFAULT_FLAGS if flags == youth_synth.SURVEY_FLAGS else youth_synth.SURVEY_FLAGS
    _both(youth_synth.pairs(i, 1, W, H, flags=other)[1][0], t0, t2)


def test_filter_hand_case_borders_and_zeros():
    out = _both(hand_case(), 40, 1000)
    assert out[3, 3] == 32725 and out[3, 4] == 32759 and out[0, 0] == -5 and out[7, 7] == 0
    assert zlib.crc32(out.tobytes()) == 1648779394
    rng = np.random.default_rng(5)
    for H, W in ((3, 3), (3, 5)):          # all border
        d = (1500 + rng.integers(-6, 7, size=(H, W))).astype(np.int16)
        d[1, 1] = 0
        for t0, t2 in PARAMS:
            _both(d, t0, t2)
    z = np.zeros((16, 24), np.int16)
    assert not _both(z, 8, 96).any()
    # the full int16 range, negatives and the clamp included
    full = rng.integers(-32768, 32768, size=(40, 68)).astype(np.int16)
    _both(full, 255, 1000)
    near = (32700 + rng.integers(-200, 68, size=(33, 70))).astype(np.int16)
    _both(near, 255, 1000)


def test_filter_batch_frames_do_not_leak():
    """Three different frames in one call: frame f's halo must not read frame
    f - 1's last rows or frame f + 1's first rows."""
    for W, H in ((24, 16), (97, 53)):
        a = youth_synth.pairs(5, 1, W, H, flags=youth_synth.SURVEY_FLAGS)[0][0]
        batch = np.stack([a, (a[::-1] + 40).astype(np.int16), np.where(a > 0, a + 3, a).astype(np.int16)])
        want = _both(batch, 8, 96)
        for f in range(3):
            assert np.array_equal(want[f], filter_truth(batch[f], 8, 96))


def test_filter_unaligned_pointers_and_640x480():
    # a 97x53 input one int16 past an aligned base, and an odd output base
    src = kat_frame("default97")
    H, W = src.shape
    buf = torch.zeros(H * W + 8, dtype=torch.int16, device="cuda")
    buf[1:1 + H * W] = torch.from_numpy(src).cuda().reshape(-1)
    d_in = buf[1:1 + H * W].view(H, W)
    assert d_in.data_ptr() % 4 == 2
    obuf = torch.zeros(H * W + 8, dtype=torch.int16, device="cuda")
    d_out = obuf[3:3 + H * W].view(H, W)
    youth_filter.depth_filter_device(d_in, d_out, 8, 96)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), filter_truth(src, 8, 96))
    assert not obuf[:3].any() and not obuf[3 + H * W:].any()
    # a width that is a multiple of 4 on a base that is not 8-byte aligned: scalar path
    s160 = kat_frame("survey160")
    H, W = s160.shape
    buf = torch.zeros(H * W + 8, dtype=torch.int16, device="cuda")
    buf[1:1 + H * W] = torch.from_numpy(s160).cuda().reshape(-1)
    got = youth_filter.depth_filter_device(buf[1:1 + H * W].view(H, W), None, 8, 96)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), filter_truth(s160, 8, 96))
    # the workload's size on the vector path; t0 = None passes NULL (the defaults)
    big = youth_synth.pairs(2, 1, 640, 480, flags=youth_synth.SURVEY_FLAGS)[0][0]
    want = filter_truth(big)
    d = torch.from_numpy(big).cuda()
    assert d.data_ptr() % 8 == 0
    got = youth_filter.depth_filter_device(d, None, None)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(youth_filter.depth_filter_host(big, None), want)
    assert int((want != big).sum()) > 100000


def test_filter_bad_arguments_then_a_valid_call():
    src = kat_frame("survey24")
    d = torch.from_numpy(src).cuda()
    out = torch.empty_like(d)
    lib = youth_filter.load_library()
    two = torch.zeros(2 * src.size, dtype=torch.int16, device="cuda")
    cases = [
        lambda: youth_filter.depth_filter_device(d, d, 8, 96),                       # the same buffer
        lambda: youth_filter.depth_filter_device(two[:src.size].view(src.shape),     # overlapping
                                                 two[10:10 + src.size].view(src.shape), 8, 96),
        lambda: youth_filter.depth_filter_device(d, out, 0, 96),
        lambda: youth_filter.depth_filter_device(d, out, 8, 1001),
        lambda: youth_filter.depth_filter_device(torch.zeros((8, 2), dtype=torch.int16, device="cuda")),
        lambda: youth_filter.depth_filter_host(src, 0, 96),
        lambda: youth_filter.depth_filter_host(np.zeros((8, 2), np.int16)),
    ]
    for k, call in enumerate(cases):
        with pytest.raises(youth_icp.IcpError) as e:
            call()
        assert e.value.code == youth_icp.YOUTH_EINVAL, k
        assert (lib.youth_depth_filter_last_error() or b"").decode().strip(), k
    youth_filter.depth_filter_device(d, out, 8, 96)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), filter_truth(src, 8, 96))
    assert np.array_equal(youth_filter.depth_filter_host(src, 8, 96), filter_truth(src, 8, 96))


# ------------------------------------------------------------- the tracker --

@pytest.mark.parametrize("spec", ["survey", "fma"])
@pytest.mark.parametrize("W,H", [(160, 120), (97, 53)])
def test_tracker_with_filter_matches_oracle_on_filtered_frames(W, H, spec):
    oracle.set_spec(spec)
    try:
        frames, _ = youth_synth.sequence(11, 6, W, H)
        filt = filter_truth(frames, 8, 96)
        K = youth_icp.default_intrinsics(W, H)
        with youth_icp.IcpContext(W, H, 8, K=K, spec=spec) as off:
            assert off.depth_filter is None
            plain = [off.track_frame(f) for f in frames]
        with youth_icp.IcpContext(W, H, 8, K=K, spec=spec) as ctx:
            ctx.set_depth_filter(8, 96)
            assert ctx.depth_filter == (8, 96)
            got = [ctx.track_frame(f) for f in frames]
        assert not got[0][2] and np.array_equal(got[0][0], np.eye(4))
        for k in range(1, len(frames)):
            T64, _, sto, _ = oracle.align(filt[k], filt[k - 1])
            assert got[k][2] and got[k][1] == sto, k
            assert _pose_err(got[k][0], T64) <= POSE_TOL, k
        assert any(not np.array_equal(got[k][0], plain[k][0]) for k in range(1, len(frames)))
    finally:
        oracle.set_spec("survey")


def test_tracker_invariants_hold_with_the_filter_on():
    W, H = 160, 120
    frames, _ = youth_synth.sequence(11, 9, W, H)
    K = youth_icp.default_intrinsics(W, H)
    with youth_icp.IcpContext(W, H, 16, K=K) as off:
        off.track_set_batch(8)
        plain = [off.track_frame(f) for f in frames]
    with youth_icp.IcpContext(W, H, 16, K=K) as ref:
        ref.track_set_batch(8)
        ref.set_depth_filter(8, 96)
        want = [ref.track_frame(f) for f in frames]
        # realign reproduces the tracked pose
        for k in (1, 4, 8):
            T, st = ref.track_realign(frames[k - 1], frames[k])
            assert st == want[k][1] and np.array_equal(T, want[k][0]), k
    Tw = np.stack([w[0] for w in want[1:]])
    sw = np.array([w[1] for w in want[1:]], np.int32)
    assert not np.array_equal(Tw, np.stack([p[0] for p in plain[1:]]))
    with youth_icp.IcpContext(W, H, 16, K=K) as ctx:
        ctx.track_set_batch(8)
        ctx.set_depth_filter(8, 96)
        Tb, stb = ctx.track_host_sequence(frames)          # micro-batches of 8
        assert ctx.track_chained() >= 1
        assert np.array_equal(Tb, Tw) and np.array_equal(stb, sw)
        # the same from page-locked buffers, read in place
        ctx.track_reset()
        pinned = [youth_icp.PinnedFrame(H, W) for _ in frames]
        try:
            for p, f in zip(pinned, frames):
                p.array[:] = f
            ctx.track_submit_pinned(pinned[:1])
            ctx.track_submit_pinned(pinned[1:9])
            # the switch is refused with frames in flight; nothing changes
            for args in ((None,), (8, 96), (40, 1000)):
                with pytest.raises(youth_icp.IcpError) as e:
                    ctx.set_depth_filter(*args)
                assert e.value.code == youth_icp.YOUTH_EINVAL
            assert ctx.depth_filter == (8, 96)
            got = [ctx.track_collect() for _ in frames]
        finally:
            for p in pinned:
                p.close()
        assert np.array_equal(np.stack([g[0] for g in got[1:]]), Tw)
        assert [g[1] for g in got[1:]] == list(sw)
        # out-of-range parameters are refused, the filter stays as it was
        for bad in ((0, 96), (256, 96), (8, 1001), (8, -1)):
            with pytest.raises(youth_icp.IcpError):
                ctx.set_depth_filter(*bad)
        assert ctx.depth_filter == (8, 96)
        # off again: today's bits, and the held reference was kept
        ctx.set_depth_filter(None)
        assert ctx.depth_filter is None
        ctx.track_reset()
        again = [ctx.track_frame(f) for f in frames]
        for a, p in zip(again, plain):
            assert np.array_equal(a[0], p[0]) and a[1] == p[1] and a[2] == p[2]
        ctx.set_depth_filter(8, 96)
        T, st, has = ctx.track_frame(frames[0])            # still a reference: frame 8, raw
        assert has


def test_device_api_is_not_filtered():
    W, H = 160, 120
    frames, _ = youth_synth.sequence(11, 4, W, H)
    K = youth_icp.default_intrinsics(W, H)
    d = torch.from_numpy(frames).cuda()
    src, dst = d[1:4].contiguous(), d[0:3].contiguous()
    with youth_icp.IcpContext(W, H, 8, K=K) as off:
        off.align_pairs_device(src.data_ptr(), dst.data_ptr(), 3)
        off.sync()
        T_off, _, st_off = off.get_poses(3)
    with youth_icp.IcpContext(W, H, 8, K=K) as ctx:
        ctx.set_depth_filter(8, 96)
        ctx.align_pairs_device(src.data_ptr(), dst.data_ptr(), 3)
        ctx.sync()
        T_on, _, st_on = ctx.get_poses(3)
        assert np.array_equal(T_on, T_off) and np.array_equal(st_on, st_off)
        # the caller filters its own buffers: the tracker's filtered pose
        f = youth_filter.depth_filter_device(d, None, 8, 96)
        torch.cuda.synchronize()
        fs, fd = f[1:4].contiguous(), f[0:3].contiguous()
        ctx.align_pairs_device(fs.data_ptr(), fd.data_ptr(), 3)
        ctx.sync()
        T_f, _, st_f = ctx.get_poses(3)
        tracked = [ctx.track_frame(x) for x in frames]
    for k in range(3):
        assert st_f[k] == tracked[k + 1][1]
        assert _pose_err(T_f[k], tracked[k + 1][0]) <= CROSS_PATH_TOL, k
    assert not np.array_equal(T_f, T_off)


# -------------------------------------------------------------- the drop-in --

_CHILD = r"""
import sys
import numpy as np
import youth_icp
import youth_synth
cfg, out = sys.argv[1], sys.argv[2]
frames, _ = youth_synth.sequence(0, 6)
youth_icp.initSlamModule(cfg)
try:
    for k in range(6):
        assert youth_icp.processSlamFrame(frames[k], None, 640, 480, 100 + k) == 1
    assert youth_icp.slam_wait_idle(30000) == 1
    ts, T = youth_icp.slam_trajectory()
finally:
    youth_icp.stopSlamModule()
np.savez(out, ts=ts, T=T)
"""


def _mat_mul4(A, B):
    """slam_api.cpp's composition, sum by sum."""
    C = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            s = 0.0
            for k in range(4):
                s += float(A[i, k]) * float(B[k, j])
            C[i, j] = s
    return C


def _composed(filter_params):
    """The trajectory of a tracker like the SLAM worker's (16 slots, planned
    for micro-batches of 8, the YAML's intrinsics)."""
    frames, _ = youth_synth.sequence(0, 6)
    K = youth_icp.parse_camera_yaml(CFG)[0]
    with youth_icp.IcpContext(640, 480, 2 * youth_icp.TRACK_MAX_BATCH, K=K) as ctx:
        ctx.track_set_batch(youth_icp.TRACK_MAX_BATCH)
        if filter_params:
            ctx.set_depth_filter(*filter_params)
        rel = [ctx.track_frame(f) for f in frames]
    acc, out = np.eye(4), []
    for k, (T, st, has) in enumerate(rel):
        assert st == 0, (k, st)
        acc = _mat_mul4(acc, T) if has else np.eye(4)
        out.append(acc.copy())
    return np.stack(out)


def _run_child(tmp_path, tag, value):
    out = str(tmp_path / f"{tag}.npz")
    env = {k: v for k, v in os.environ.items()
           if k not in ("YOUTH_ICP_DEPTH_FILTER", "YOUTH_SLAM_TRACK_BATCH")
           and not k.startswith("YOUTH_SLAM_MAP_")}
    env.update(YOUTH_ICP_DEPTH_FILTER=value,
               PYTHONPATH=os.pathsep.join([PKG, ORACLE] + [p for p in sys.path if p]))
    r = subprocess.run([sys.executable, "-c", _CHILD, CFG, out], env=env, timeout=120,
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    z = np.load(out, allow_pickle=False)
    return z["ts"], z["T"], r.stderr


def test_slam_drop_in_takes_the_filter_from_the_environment(tmp_path):
    """The worker's context reads YOUTH_ICP_DEPTH_FILTER when it is created,
    so each setting runs in a fresh child process."""
    on, off = _composed((8, 96)), _composed(None)
    assert not np.array_equal(on, off)
    ts, T, err = _run_child(tmp_path, "on", "8,96")
    assert list(ts) == [100 + k for k in range(6)]
    assert np.array_equal(T.reshape(-1, 4, 4), on)
    assert "YOUTH_ICP_DEPTH_FILTER" not in err
    ts, T, err = _run_child(tmp_path, "bogus", "bogus")
    assert list(ts) == [100 + k for k in range(6)]
    assert np.array_equal(T.reshape(-1, 4, 4), off)
    notice = [ln for ln in err.splitlines() if "YOUTH_ICP_DEPTH_FILTER" in ln]
    assert len(notice) == 1 and "bogus" in notice[0] and "off" in notice[0]


# ---------------------------------------------------------------- accuracy --

def test_accuracy_on_the_gpu_at_survey_noise():
    """8 pairs at SURVEY noise, 640x480 (dst tracked first, then src): with
    the filter every pair is within 0.05 degrees and 2 mm of T_gt and within
    1e-5 of the oracle on the filtered frames; without it the median rotation
    error is >= 0.2 degrees."""
    src, dst, T_gt = youth_synth.pairs(0, 8, 640, 480, flags=youth_synth.SURVEY_FLAGS)
    fs, fd = filter_truth(src), filter_truth(dst)
    raw_rot = []
    with youth_icp.IcpContext(640, 480, 2) as ctx:
        for on in (True, False):
            ctx.set_depth_filter(8, 96) if on else ctx.set_depth_filter(None)
            for p in range(8):
                ctx.track_reset()
                ctx.track_frame(dst[p])
                T, st, has = ctx.track_frame(src[p])
                assert has
                rot, trans = pose_error(T, T_gt[p])
                print(f"pair {p} filter {'on' if on else 'off'}: {rot:.4f} deg {trans:.3f} mm")
                if on:
                    assert rot <= 0.05 and trans <= 2.0, (p, rot, trans)
                    T64, _, sto, _ = oracle.align(fs[p], fd[p], iters=10)
                    assert st == sto and _pose_err(T, T64) <= POSE_TOL, p
                else:
                    raw_rot.append(rot)
    assert float(np.median(raw_rot)) >= 0.2
