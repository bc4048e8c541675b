"""GPU parity tests: the HIP path (through the C-ABI) against the C oracle.

Bar:
  * XYZ, normals, association indices: bit-exact (given the same fp32 pose);
  * normal-equation sums: fp64, differ only by summation order -> rel 1e-12;
  * recovered SE(3) pose: max |T_gpu - T_cpu| over the 3x4 entries <= 1e-5
    (north_star tolerance; observed ~1e-15).
"""
import os
import tempfile

import numpy as np
import pytest

import oracle
import youth_icp
import youth_synth
from conftest import GOLDEN, lanes_of, oracle_like

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-5


def _load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def _K(arr):
    return youth_icp.Intrinsics(*[float(v) for v in arr])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _pose_err(A, B):
    return float(np.abs(np.asarray(A)[:3, :4] - np.asarray(B)[:3, :4]).max())


# --------------------------------------------------------------- prepare --
def test_backproject_kat_on_gpu():
    table = _load("kat_backproject")["table"].tolist()
    for W, H in {(r[0], r[1]) for r in table}:
        depth = np.zeros((H, W), np.int16)
        rows = [r for r in table if (r[0], r[1]) == (W, H)]
        for _, _, u, v, d, *_ in rows:
            depth[v, u] = d
        with youth_icp.IcpContext(W, H, 2) as ctx:
            X, Y, Z, *_ = ctx.prepare(depth, want_normals=False)
        for _, _, u, v, d, xb, yb, zb in rows:
            got = tuple(int(_bits(A[0, v, u]).item()) for A in (X, Y, Z))
            assert got == (xb, yb, zb), (W, H, u, v, d)


@pytest.mark.parametrize("W,H", [(640, 480), (97, 53), (64, 16), (1280, 960), (65, 17)])
def test_prepare_bit_exact(W, H):
    src, dst, _ = youth_synth.pairs(11, 2, W, H)
    frames = np.concatenate([src, dst])
    # exercise invalid / extreme raw values too
    frames[0, 0, :5] = [-1, -32768, 32767, 0, 1]
    with youth_icp.IcpContext(W, H, 4) as ctx:
        X, Y, Z, NX, NY, NZ = ctx.prepare(frames, want_normals=True)
    for f in range(4):
        oX, oY, oZ = oracle.backproject(frames[f])
        oN = oracle.normals(oX, oY, oZ)
        assert np.array_equal(_bits(X[f]), _bits(oX))
        assert np.array_equal(_bits(Y[f]), _bits(oY))
        assert np.array_equal(_bits(Z[f]), _bits(oZ))
        for g, o in zip((NX[f], NY[f], NZ[f]), oN):
            assert np.array_equal(_bits(g), _bits(o)), f


@pytest.mark.parametrize("W,H,n", [(640, 480, 12), (1280, 960, 3), (96, 64, 40), (97, 53, 3)])
def test_prepare_records_align_path_bit_exact(W, H, n):
    """The align path's record kernel as an align runs it (no X/Y/Z planes;
    wide and narrow halo loads, many tiles) gives the oracle's normals bit for
    bit, and the same as the stage-level call that also stores the planes."""
    src, dst, _ = youth_synth.pairs(21, (n + 1) // 2, W, H)
    frames = np.concatenate([src, dst])[:n]
    frames[0, 1, :5] = [-1, -32768, 32767, 0, 1]
    with youth_icp.IcpContext(W, H, n) as ctx:
        rec = ctx.prepare(frames, want_normals=True, want_xyz=False)
        ref = ctx.prepare(frames, want_normals=True, want_xyz=True)
    for f in range(n):
        oN = oracle.normals(*oracle.backproject(frames[f]))
        for g, r, o in zip(rec[3:], ref[3:], oN):
            assert np.array_equal(_bits(g[f]), _bits(o)), f
            assert np.array_equal(_bits(g[f]), _bits(r[f])), f


@pytest.mark.parametrize("name", ["pair_80x60", "pair_160x120", "pair_97x53"])
def test_prepare_matches_golden(name):
    g = _load(name)
    K = _K(g["K"])
    H, W = g["src"].shape
    with youth_icp.IcpContext(W, H, 2, K=K) as ctx:
        out = ctx.prepare(np.stack([g["src"], g["dst"]]), want_normals=True)
    assert np.array_equal(_bits(np.stack(out[:3])[:, 0]), _bits(g["src_xyz"]))
    assert np.array_equal(_bits(np.stack(out[:3])[:, 1]), _bits(g["dst_xyz"]))
    assert np.array_equal(_bits(np.stack(out[3:])[:, 1]), _bits(g["dst_nrm"]))


# ---------------------------------------------------------- association --
@pytest.mark.parametrize("name", ["pair_80x60", "pair_160x120", "pair_97x53"])
def test_assoc_and_reduce_match_golden(name):
    g = _load(name)
    K = _K(g["K"])
    H, W = g["src"].shape
    with youth_icp.IcpContext(W, H, 2, K=K, dist_thresh=float(g["dist_thresh"]),
                              reduction="exact") as ctx:     # the fixtures' reduction
        I12 = np.eye(4, dtype=np.float32)[:3]
        assoc, neq = ctx.reduce(g["src"], g["dst"], I12)
        assert np.array_equal(assoc, g["idx_identity"])
        np.testing.assert_allclose(neq, g["neq_identity"], rtol=1e-12, atol=1e-12)
        assoc, _ = ctx.reduce(g["src"], g["dst"], g["T32"])
        assert np.array_equal(assoc, g["idx_final"])


def test_assoc_bit_exact_every_iteration_640x480():
    """Index bit-exactness given the SAME fp32 pose: feed the oracle's T_k."""
    src, dst, _ = youth_synth.pairs(0, 1)
    src, dst = src[0], dst[0]
    K = oracle.viewer_K(640, 480)
    with youth_icp.IcpContext(640, 480, 2) as ctx:
        T = np.eye(4)
        for it in range(10):
            T32 = T[:3].astype(np.float32)
            g_idx, g_neq = ctx.reduce(src, dst, T32)
            o_idx = oracle.associate(src, dst, T32, K)
            with oracle_like(ctx):
                o_neq = oracle.reduce(src, dst, T32, K)
            assert np.array_equal(g_idx, o_idx), it
            np.testing.assert_allclose(g_neq, o_neq, rtol=1e-11, atol=1e-9)
            xi, st = oracle.solve(o_neq)
            assert st == 0
            T = oracle.se3_exp(xi) @ T


def test_solve_matches_oracle():
    src, dst, _ = youth_synth.pairs(5, 1, 320, 240)
    K = oracle.viewer_K(320, 240)
    neq = oracle.reduce(src[0], dst[0], np.eye(4, dtype=np.float32)[:3], K)
    xi, st = oracle.solve(neq)
    T0 = np.eye(4)
    T0[:3, 3] = [0.01, -0.02, 0.03]
    with youth_icp.IcpContext(320, 240, 2) as ctx:
        Tg, stg = ctx.solve(neq, T0)
        assert stg == st == 0
        assert np.abs(Tg - oracle.se3_exp(xi) @ T0).max() < 1e-13
        bad = np.zeros(29)
        bad[28] = 3
        Tb, stb = ctx.solve(bad, T0)
        assert stb == youth_icp.STATUS_FEW_MATCHES and np.array_equal(Tb, T0)
        bad[28] = 100
        Tb, stb = ctx.solve(bad, T0)
        assert stb == youth_icp.STATUS_DEGENERATE and np.array_equal(Tb, T0)


def test_solve_random_systems_match_oracle():
    """Spec a10's block-elimination solve on the device against the oracle on
    400 systems: sums of rank 1-8 outer products of rotation-and-translation
    Jacobians at scales 2^-20 .. 2^20 (rank < 6 is singular: DEGENERATE), a
    few with fewer than 6 matches.  Statuses equal; updated poses equal the
    oracle's exp(xi) T0 within 1e-13 (tools/solvebench checks xi bit for bit
    on 262,144 such systems)."""
    rng = np.random.default_rng(17)
    T0 = np.eye(4)
    T0[:3, 3] = [0.01, -0.02, 0.03]
    n_ok = n_deg = 0
    with youth_icp.IcpContext(64, 48, 2) as ctx:
        for c in range(400):
            rank = 1 + c % 8
            sc = 2.0 ** ((c // 8) % 41 - 20)
            p = rng.normal(size=(rank * 3, 3)) * 2.0
            nrm = rng.normal(size=(rank * 3, 3))
            J = np.hstack([np.cross(p, nrm), nrm]) * sc
            J[rank:] = 0.0
            A = J.T @ J
            neq = np.zeros(29)
            neq[:21] = A[np.triu_indices(6)]
            neq[21:27] = rng.normal(size=6) * 1e-3 * sc * sc
            neq[28] = 3.0 if c % 97 == 5 else 1000.0
            xi, st = oracle.solve(neq)
            Tg, stg = ctx.solve(neq, T0)
            assert stg == st, c
            if st == 0:
                n_ok += 1
                assert np.abs(Tg - oracle.se3_exp(xi) @ T0).max() < 1e-13, c
            else:
                n_deg += 1
                assert np.array_equal(Tg, T0), c
    assert n_ok > 100 and n_deg > 100


# ----------------------------------------------------------- full align --
def test_align_batch_640x480_matches_oracle():
    n = 8
    src, dst, Tgt = youth_synth.pairs(0, n)
    Tg, assoc = youth_icp.align_batch(src, dst, iters=10, want_assoc=True)
    for p in range(n):
        T64, T32, st, _ = oracle.align(src[p], dst[p], iters=10)
        assert st == 0
        assert _pose_err(Tg[p], T64) <= POSE_TOL, p
        assert np.array_equal(assoc[p], oracle.associate(src[p], dst[p], Tg[p][:3]))


def _per_chunk(src, dst, k, iters=10):
    """The poses of the batch aligned as separate unpipelined calls of k pairs
    (the last one ragged): the launch shapes a pipelined call of chunk k runs."""
    out = []
    for a in range(0, src.shape[0], k):
        T, _ = youth_icp.align_batch(src[a:a + k], dst[a:a + k], iters=iters)
        out.append(T)
    return np.concatenate(out)


@pytest.mark.parametrize("chunk", ["0", "8", "5"])
def test_align_batch_pipelined_chunks(chunk, monkeypatch):
    """Host-buffer batch API with H2D of chunk k+1 overlapping the align of
    chunk k (YOUTH_ICP_BATCH_CHUNK; 21 pairs leaves a ragged last chunk):
    bit-identical to the same chunks aligned by separate unpipelined calls
    (spec a9's lane sums depend on the launch shape, i.e. on the pairs per
    launch, so that is the reference with the same shapes), a repeat
    bit-identical, and within 1e-5 of the oracle."""
    n = 21
    src, dst, _ = youth_synth.pairs(100, n, 160, 120)
    monkeypatch.setenv("YOUTH_ICP_BATCH_CHUNK", "0")
    T_ref = _per_chunk(src, dst, int(chunk) or n)
    monkeypatch.setenv("YOUTH_ICP_BATCH_CHUNK", chunk)
    T_chk, _ = youth_icp.align_batch(src, dst, iters=10)
    T_again, _ = youth_icp.align_batch(src, dst, iters=10)
    assert np.array_equal(T_chk, T_again)
    assert np.array_equal(T_chk, T_ref)
    for p in (0, 7, 8, 20):
        T64, _, st, _ = oracle.align(src[p], dst[p], iters=10)
        assert _pose_err(T_chk[p], T64) <= POSE_TOL, p


def test_align_batch_default_chunks_ragged_tail(monkeypatch):
    """Default pipelining at 40 pairs: chunks of 16, 16 and 8 (persistent
    kernel, then a cooperative tail on the same context, workspace reserved
    for both before the loop) equal those chunks aligned by separate
    unpipelined calls bit for bit, and the oracle within 1e-5."""
    n = 40
    src, dst, _ = youth_synth.pairs(200, n)
    monkeypatch.delenv("YOUTH_ICP_BATCH_CHUNK", raising=False)
    T_chk, _ = youth_icp.align_batch(src, dst, iters=10)
    monkeypatch.setenv("YOUTH_ICP_BATCH_CHUNK", "0")
    assert np.array_equal(T_chk, _per_chunk(src, dst, 16))
    for p in (0, 15, 16, 32, 39):
        T64, _, st, _ = oracle.align(src[p], dst[p], iters=10)
        assert st == 0 and _pose_err(T_chk[p], T64) <= POSE_TOL, p


@pytest.mark.parametrize("devices", [None, [0]])
def test_align_batch_multi_matches_single_device(devices):
    """youth_icp_align_batch_multi (one host thread + context per device,
    contiguous shards, poses written into the caller's rows) on this box's
    device(s): poses equal youth_icp_align_batch's bit for bit, the oracle's
    within 1e-5, and per-pair status reported (a pair without source pixels
    is YOUTH_STATUS_FEW_MATCHES with the identity pose).  N > 1 devices:
    unmeasured here (one-GPU boxes)."""
    n = 37
    src, dst, _ = youth_synth.pairs(400, n, 160, 120)
    src[5] = 0
    T_m, st = youth_icp.align_batch_multi(src, dst, iters=10, devices=devices)
    T_1, _ = youth_icp.align_batch(src, dst, iters=10)
    assert np.array_equal(T_m, T_1)
    assert st[5] == youth_icp.STATUS_FEW_MATCHES and np.array_equal(T_m[5], np.eye(4))
    assert not np.delete(st, 5).any()
    for p in (0, 6, 36):
        T64, _, sto, _ = oracle.align(src[p], dst[p], iters=10)
        assert sto == 0 and _pose_err(T_m[p], T64) <= POSE_TOL, p
    with pytest.raises(youth_icp.IcpError):
        youth_icp.align_batch_multi(src, dst, devices=[0, 0])
    with pytest.raises(youth_icp.IcpError):
        youth_icp.align_batch_multi(src, dst, devices=[youth_icp.device_count()])


@pytest.mark.parametrize("n", [1, 40])
def test_large_step_rodrigues_branch(n):
    """Spec a10 above theta = 5 deg (theta^2 >= 2^-7): the SE(3) update leaves
    the Taylor form for sqrt/sincos (OCML on the GPU, libm in the oracle: may
    differ in an ulp).  T_init is 7 deg off the true motion and the gate is
    opened to 1 m, so the Gauss-Newton step is ~8 deg; one iteration (from
    there projective ICP leaves its basin, and a chaotic trajectory is no
    parity case), both kernel paths (n = 1: cooperative, n = 40: persistent);
    pose within the north-star tolerance, and the wave solve's large-angle
    branch also through the single-lane solve entry point."""
    import torch  # plumbing only: device memory
    W, H = 320, 240
    src, dst, Tgt = youth_synth.pairs(300, n, W, H)
    axis = np.array([0.3, 1.0, 0.2])
    axis /= np.linalg.norm(axis)
    R0 = oracle.se3_exp(np.r_[axis * np.deg2rad(7.0), 0.0, 0.0, 0.0])
    T_init = np.stack([R0 @ Tgt[p] for p in range(n)])
    ds = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    dd = torch.from_numpy(np.ascontiguousarray(dst)).cuda()
    torch.cuda.synchronize()
    with youth_icp.IcpContext(W, H, max(n, 2), iters=1, dist_thresh=1.0) as ctx:
        ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), n, T_init=T_init)
        ctx.sync()
        T64, _, st = ctx.get_poses(n)
    for p in sorted({0, n - 1}):
        T64o, _, sto, _ = oracle.align(src[p], dst[p], iters=1, dist_thresh=1.0,
                                       T_init=T_init[p])
        assert st[p] == sto == 0
        step = np.arccos(np.clip((np.trace(T64o[:3, :3] @ T_init[p][:3, :3].T) - 1) / 2, -1, 1))
        assert step > np.deg2rad(5.1), np.rad2deg(step)
        assert _pose_err(T64[p], T64o) <= POSE_TOL, p
    neq = oracle.reduce(src[0], dst[0], T_init[0][:3].astype(np.float32), oracle.viewer_K(W, H),
                        dist_thresh=1.0)
    xi, st0 = oracle.solve(neq)
    assert st0 == 0 and np.linalg.norm(xi[:3]) ** 2 >= 2.0 ** -7
    with youth_icp.IcpContext(W, H, 2) as ctx:
        Tg, stg = ctx.solve(neq, T_init[0])
    assert stg == 0 and np.abs(Tg - oracle.se3_exp(xi) @ T_init[0]).max() < 1e-12


def test_context_device_api_poses_and_stats():
    n = 6
    src, dst, _ = youth_synth.pairs(20, n)
    import ctypes
    with youth_icp.IcpContext(640, 480, 2 * n) as ctx:
        # host arrays through the one-shot path, then the context getters
        Tb, _ = youth_icp.align_batch(src, dst, iters=10)
        T_init = np.tile(np.eye(4), (n, 1, 1))
        lib = youth_icp.load_library()
        # device copies via the library's own stream: use align_batch's staging
        hs = np.ascontiguousarray(src)
        hd = np.ascontiguousarray(dst)
        import torch  # plumbing only: device memory
        ds = torch.from_numpy(hs).cuda()
        dd = torch.from_numpy(hd).cuda()
        out = torch.zeros((n, 16), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), n, T_init=T_init,
                               d_T_out=out.data_ptr())
        ctx.sync()
        T64, T32, st = ctx.get_poses(n)
        cnt, r2 = ctx.get_stats(n, 10)
        Tdev = out.cpu().numpy().reshape(n, 4, 4)
        lanes = lanes_of(ctx)
        del lib, ctypes
    for p in range(n):
        with oracle_like(lanes):
            T64o, _, sto, stats = oracle.align(src[p], dst[p], iters=10)
        assert _pose_err(T64[p], T64o) <= POSE_TOL
        assert np.array_equal(Tdev[p], T32[p]) and np.array_equal(Tdev[p], Tb[p])
        assert st[p] == sto
        assert np.array_equal(cnt[p], stats[:, 0])
        np.testing.assert_allclose(r2[p], stats[:, 1], rtol=1e-9)


def test_align_1280x960_20_iters():
    src, dst, _ = youth_synth.pairs(3, 2, 1280, 960)
    K = youth_icp.default_intrinsics(1280, 960)
    Tg, _ = youth_icp.align_batch(src, dst, K=K, iters=20)
    for p in range(2):
        T64, _, st, _ = oracle.align(src[p], dst[p], iters=20)
        assert st == 0 and _pose_err(Tg[p], T64) <= POSE_TOL


@pytest.mark.parametrize("tile_src", ["1", "0"])
def test_single_pair_coop_tile_sources(tile_src, monkeypatch):
    """C2 (640x480, 10 it) and C3 (1280x960, 20 it) single pairs through
    k_icp_coop with tile-shaped source chunks (64x24 / 64x80 prep tiles, one
    per workgroup) and with contiguous ones (YOUTH_ICP_COOP_TILE_SRC=0):
    every fp64 pose within the bar of the oracle's, correspondence counts per
    iteration equal to the oracle's."""
    import torch
    monkeypatch.setenv("YOUTH_ICP_COOP_TILE_SRC", tile_src)
    for W, H, iters, G, px in ((640, 480, 10, 200, 3), (1280, 960, 20, 240, 10)):
        src, dst, _ = youth_synth.pairs(31, 1, W, H)
        ds, dd = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
        with youth_icp.IcpContext(W, H, 2, iters=iters) as ctx:
            ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), 1)
            T64, _, st = ctx.get_poses(1)
            cnt, _ = ctx.get_stats(1, iters)
            plan = ctx.get_plan()
            lanes = lanes_of(ctx)
        assert plan["kernel"] == "k_icp_coop" and plan["workgroups_per_pair"] == G
        assert plan["px_per_lane"] == px
        with oracle_like(lanes):
            To, _, sto, stats = oracle.align(src[0], dst[0], iters=iters)
        assert st[0] == sto and _pose_err(T64[0], To) <= POSE_TOL
        assert np.array_equal(cnt[0], stats[:, 0])


@pytest.mark.parametrize("name", ["pair_80x60", "pair_160x120", "pair_97x53"])
def test_align_matches_golden_pose(name):
    g = _load(name)
    Tg, _ = youth_icp.align_batch(g["src"][None], g["dst"][None], K=_K(g["K"]),
                                  iters=int(g["iters"]))
    assert _pose_err(Tg[0], g["T64"]) <= POSE_TOL


def test_identity_and_empty_edge_cases():
    src, dst, _ = youth_synth.pairs(9, 1, 160, 120)
    z = np.zeros((160 * 120,), np.int16).reshape(120, 160)
    S = np.stack([dst[0], z, z, dst[0]])
    D = np.stack([dst[0], z, dst[0], z])
    with youth_icp.IcpContext(160, 120, 8, iters=3) as ctx:
        import torch
        ds = torch.from_numpy(S).cuda()
        dd = torch.from_numpy(D).cuda()
        torch.cuda.synchronize()
        ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), 4)
        T64, _, st = ctx.get_poses(4)
    assert np.array_equal(T64[0], np.eye(4)) and st[0] == 0       # identical frames
    for p in (1, 2, 3):                                             # empty source/target
        assert np.array_equal(T64[p], np.eye(4)) and st[p] == youth_icp.STATUS_FEW_MATCHES


def test_sequence_api_matches_oracle():
    g = _load("seq_128x96")
    frames = g["frames"]
    n = frames.shape[0]
    import torch
    with youth_icp.IcpContext(128, 96, n, K=_K(g["K"]), iters=int(g["iters"])) as ctx:
        d = torch.from_numpy(frames).cuda()
        torch.cuda.synchronize()
        ctx.align_sequence_device(d.data_ptr(), n)
        T64, _, st = ctx.get_poses(n - 1)
    for k in range(n - 1):
        assert _pose_err(T64[k], g["T_rel"][k]) <= POSE_TOL, k


def test_sequence_c5_workload_640x480():
    """Config C5 at its frame size: a 201-frame 640x480 synthetic sequence
    (seed 0x5EED1000) through align_sequence_device (every frame
    prepared once, 200 relative poses in one call).  EVERY relative pose
    within 1e-5 of the oracle (OpenMP over pairs); per-iteration
    correspondence counts equal to the oracle's and association indices at
    the final pose bit-exact on sampled pairs."""
    import torch
    F = 201
    frames, _ = youth_synth.sequence(0, F)
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    with youth_icp.IcpContext(640, 480, F - 1) as ctx:
        ctx.align_sequence_device(d.data_ptr(), F)
        ctx.sync()
        T64, T32, st = ctx.get_poses(F - 1)
        cnt, _ = ctx.get_stats(F - 1, 10)
        lanes = lanes_of(ctx)
        with oracle_like(lanes):
            T_cpu, st_cpu = oracle.align_batch(frames[1:], frames[:-1], iters=10,
                                               n_threads=min(16, os.cpu_count() or 1))
        assert np.array_equal(st, st_cpu) and not st.any()
        err = [_pose_err(T64[k], T_cpu[k]) for k in range(F - 1)]
        assert max(err) <= POSE_TOL, int(np.argmax(err))
        K = oracle.viewer_K(640, 480)
        for k in (0, 1, 77, 150, F - 2):
            with oracle_like(lanes):
                _, _, _, stats = oracle.align(frames[k + 1], frames[k], iters=10)
            assert np.array_equal(cnt[k], stats[:, 0]), k
            g_idx, _ = ctx.reduce(frames[k + 1], frames[k], T32[k][:3])
            assert np.array_equal(g_idx, oracle.associate(frames[k + 1], frames[k], T32[k][:3], K))


def test_sequence_c5_full_length_one_call():
    """Config C5 at its real length: the 1000-frame
    640x480 sequence (seed 0x5EED1000) in ONE align_sequence_device call: 999
    pairs, so the 3072-chunk work geometry and ~4.9 GB of target records (pair
    880's frame lies past 2^32 bytes of records).  Reference anchor: the
    serial frame-to-frame loop SLAM.cpp:32-63.  EVERY relative pose within
    1e-5 of the oracle; per-iteration correspondence counts equal to the
    oracle's on pairs 0/255/256/511/880/998; association indices at the final
    fp32 pose bit-exact on pairs 0/880/998."""
    import torch
    F = 1000
    frames, _ = youth_synth.sequence(0, F)
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    with youth_icp.IcpContext(640, 480, F - 1) as ctx:
        ctx.align_sequence_device(d.data_ptr(), F)
        ctx.sync()
        T64, T32, st = ctx.get_poses(F - 1)
        cnt, _ = ctx.get_stats(F - 1, 10)
        lanes = lanes_of(ctx)
    del d
    with oracle_like(lanes):
        T_cpu, st_cpu = oracle.align_batch(frames[1:], frames[:-1], iters=10,
                                           n_threads=min(16, os.cpu_count() or 1))
    assert np.array_equal(st, st_cpu) and not st.any()
    err = [_pose_err(T64[k], T_cpu[k]) for k in range(F - 1)]
    assert max(err) <= POSE_TOL, (int(np.argmax(err)), max(err))
    K = oracle.viewer_K(640, 480)
    with youth_icp.IcpContext(640, 480, 2) as one:
        for k in (0, 255, 256, 511, 880, 998):
            with oracle_like(lanes):
                _, _, _, stats = oracle.align(frames[k + 1], frames[k], iters=10)
            assert np.array_equal(cnt[k], stats[:, 0]), k
            if k in (0, 880, 998):
                g_idx, _ = one.reduce(frames[k + 1], frames[k], T32[k][:3])
                assert np.array_equal(
                    g_idx, oracle.associate(frames[k + 1], frames[k], T32[k][:3], K)), k


def test_track_frame_matches_oracle():
    frames, _ = youth_synth.sequence(0, 5)
    with youth_icp.IcpContext(640, 480, 2) as ctx:
        T, st, has = ctx.track_frame(frames[0])
        assert not has and np.array_equal(T, np.eye(4))
        for k in range(1, 5):
            T, st, has = ctx.track_frame(frames[k])
            T64, _, sto, _ = oracle.align(frames[k], frames[k - 1])
            assert has and st == sto and _pose_err(T, T64) <= POSE_TOL
        ctx.track_reset()
        T, st, has = ctx.track_frame(frames[4])
        assert not has


def test_track_submit_collect_pipelined():
    """Two frames in flight (the SLAM worker's pattern): every collected
    result equals the synchronous track_frame sequence bit for bit, in any
    submit/collect interleaving; a reset with frames in flight starts a new
    sequence at the next submission; misuse is refused (EINVAL)."""
    frames, _ = youth_synth.sequence(3, 9 + youth_icp.TRACK_MAX_IN_FLIGHT)
    with youth_icp.IcpContext(640, 480, 2) as ref:
        want = [ref.track_frame(f) for f in frames[:9]]
    with youth_icp.IcpContext(640, 480, 2) as ctx:
        with pytest.raises(youth_icp.IcpError):
            ctx.track_collect()                              # nothing in flight
        got = []
        order = "SCSSCCSSSCSCSCCSCC"   # S = submit next frame, C = collect oldest (<= 4 in flight)
        k = 0
        for op in order:
            if op == "S":
                ctx.track_submit(frames[k])
                k += 1
            else:
                got.append(ctx.track_collect())
        assert k == len(want) and len(got) == len(want) and ctx.track_pending() == 0
        for (Tg, sg, hg), (Tw, sw, hw) in zip(got, want):
            assert np.array_equal(Tg, Tw) and sg == sw and hg == hw
        D = youth_icp.TRACK_MAX_IN_FLIGHT
        assert D == 16
        for f in range(D):
            ctx.track_submit(frames[f])
        with pytest.raises(youth_icp.IcpError):
            ctx.track_submit(frames[D])                      # one frame too many in flight
        with pytest.raises(youth_icp.IcpError):
            ctx.track_frame(frames[D])                       # frames not collected
        ctx.track_reset()                                    # frames 0 .. D-1 in flight
        _, _, h0 = ctx.track_collect()
        ctx.track_submit(frames[D])
        hs = [h0] + [ctx.track_collect()[2] for _ in range(D)]
        assert hs == [True] * D + [False]                    # frame D starts a new sequence
        T, st, has = ctx.track_frame(frames[D + 1])
        T64, _, sto, _ = oracle.align(frames[D + 1], frames[D])
        assert has and st == sto and _pose_err(T, T64) <= POSE_TOL
        # the library's own loop over a host sequence: the same results
        ctx.track_reset()
        Tseq, stseq = ctx.track_host_sequence(frames[:9])
        assert Tseq.shape[0] == len(want) - 1 and ctx.track_pending() == 0
        for k in range(len(want) - 1):
            assert np.array_equal(Tseq[k], want[k + 1][0]) and stseq[k] == want[k + 1][1]
        Tmore, _ = ctx.track_host_sequence(frames[:2])       # continues from frame 8
        assert Tmore.shape[0] == 2


# ------------------------------------------------------- SLAM.h drop-in --
def test_slam_api_end_to_end():
    frames, Twc = youth_synth.sequence(0, 8)
    cfg = os.path.join(GOLDEN, "astra_camera.yaml")
    youth_icp.initSlamModule(cfg, "ORBvoc.txt")
    try:
        assert youth_icp.isSlamModuleRunning() == 1
        for k in range(8):
            assert youth_icp.processSlamFrame(frames[k], None, 640, 480, 1000 + 33 * k) == 1
            assert youth_icp.slam_wait_idle(20000) == 1      # keep the queue from dropping
        ts, T = youth_icp.slam_trajectory()
        assert list(ts) == [1000 + 33 * k for k in range(8)]
        assert youth_icp.getSlamMapPoints() == int((frames[7] > 0).sum())
        # world poses = prefix product of the oracle's relative poses
        acc = np.eye(4)
        assert np.array_equal(T[0], acc)
        for k in range(1, 8):
            T64, _, _, _ = oracle.align(frames[k], frames[k - 1])
            acc = acc @ T64
            assert _pose_err(T[k], acc) <= POSE_TOL
        with tempfile.TemporaryDirectory() as td:
            base = os.path.join(td, "map")
            assert youth_icp.saveSlamMap(base) == 1
            rows = np.loadtxt(base + "_trajectory.txt")
            assert rows.shape == (8, 8) and os.path.exists(base + "_keyframes.txt")
            assert np.allclose(rows[:, 0], ts)
            assert np.allclose(rows[:, 1:4], T[:, :3, 3], atol=1e-8)
            assert np.allclose(np.linalg.norm(rows[:, 4:], axis=1), 1.0)
        youth_icp.resetSlam()
        assert youth_icp.processSlamFrame(frames[0], None, 640, 480, 5) == 1
        assert youth_icp.slam_wait_idle(20000) == 1
        ts, T = youth_icp.slam_trajectory()
        assert list(ts) == [5] and np.array_equal(T[0], np.eye(4))
    finally:
        youth_icp.stopSlamModule()
    assert youth_icp.isSlamModuleRunning() == 0
    assert youth_icp.processSlamFrame(frames[0], None, 640, 480, 0) == 0


@pytest.mark.parametrize("batch", [None, 2, 8])
def test_slam_worker_micro_batches(monkeypatch, batch):
    """A backlogged queue (9 frames pushed at once, under the reference's
    drop threshold of 10) is tracked in micro-batches of up to m frames: by
    default (batch None: m = YOUTH_TRACK_MAX_BATCH, the queue's page-locked
    buffers submitted in place) and with YOUTH_SLAM_TRACK_BATCH=m.  Every
    pose is the one the batch plan gives frame by frame (composition aside:
    world poses within 1e-12 of the prefix product of the context's relative
    poses) and within 1e-5 of the oracle's."""
    if batch is None:
        monkeypatch.delenv("YOUTH_SLAM_TRACK_BATCH", raising=False)
        batch = youth_icp.TRACK_MAX_BATCH
    else:
        monkeypatch.setenv("YOUTH_SLAM_TRACK_BATCH", str(batch))
    F = 9
    frames, _ = youth_synth.sequence(0, F)
    youth_icp.initSlamModule(os.path.join(GOLDEN, "astra_camera.yaml"), "ORBvoc.txt")
    try:
        for k in range(F):
            assert youth_icp.processSlamFrame(frames[k], None, 640, 480, 100 + k) == 1
        assert youth_icp.slam_wait_idle(20000) == 1
        ts, T = youth_icp.slam_trajectory()
        batched = youth_icp.slam_batched_frames()
    finally:
        youth_icp.stopSlamModule()
    assert list(ts) == [100 + k for k in range(F)]
    assert batched >= 2, batched
    K = youth_icp.parse_camera_yaml(os.path.join(GOLDEN, "astra_camera.yaml"))[0]
    with youth_icp.IcpContext(640, 480, 2 * batch, K=K) as ctx:
        ctx.track_set_batch(batch)
        rel = [ctx.track_frame(f)[0] for f in frames][1:]
    acc, acc_o = np.eye(4), np.eye(4)
    assert np.array_equal(T[0], acc)
    for k in range(1, F):
        acc = acc @ rel[k - 1]
        acc_o = acc_o @ oracle.align(frames[k], frames[k - 1])[0]
        assert _pose_err(T[k], acc) <= 1e-12
        assert _pose_err(T[k], acc_o) <= POSE_TOL


def test_slam_ingest_trace_accounts_for_every_frame():
    """youth_slam_trace_*: over a backlog of 30 frames pushed as a producer
    would (waiting while 10 are queued), the trace holds one push begin/end
    per frame with no pool miss (initSlamModule pre-filled the page-locked
    pool), micro-batches whose sizes add up to the frames taken, every
    submission with its five steps in order and a zero return code, one
    collect per frame, and timestamps inside the run."""
    F = 30
    frames, _ = youth_synth.sequence(3, F)
    lib = youth_icp.load_library()
    youth_icp.initSlamModule(None)
    try:
        youth_icp.slam_trace_enable(1 << 16)
        for k in range(F):
            while lib.youth_slam_queue_size() >= 10:
                pass
            assert youth_icp.processSlamFrame(frames[k], None, 640, 480, k) == 1
        assert youth_icp.slam_wait_idle(20000) == 1
        t, kind, arg = youth_icp.slam_trace_read()
        assert youth_icp.slam_trajectory()[0].size == F
    finally:
        youth_icp.slam_trace_enable(0)
        youth_icp.stopSlamModule()
    names = [youth_icp.SLAM_EVENTS[int(v)] for v in kind]
    ev = list(zip(names, (int(a) for a in arg)))
    assert names.count("push_begin") == F and names.count("push_end") == F
    assert all(a == 0 for n, a in ev if n == "push_end")          # every buffer pooled
    assert "drop" not in names
    assert sum(a for n, a in ev if n == "take") == F
    assert names.count("collect_end") == F
    subs = [i for i, n in enumerate(names) if n == "submit_begin"]
    assert len(subs) == names.count("submit_end") == names.count("take")
    for i in subs:                                  # the worker's own events are sequential
        j = names.index("submit_end", i)
        steps = [a for n, a in ev[i:j] if n == "submit_step"]
        # one tracker submission per launch (a sequence's first frame is
        # prepped by a launch of its own): steps 1..5 in order, each time
        assert steps and len(steps) % 5 == 0, steps
        assert steps == [1, 2, 3, 4, 5] * (len(steps) // 5), steps
        assert ev[j][1] == 0
    assert t.size == len(names) and np.isfinite(t).all() and 0 < t.max() - t.min() < 60


def test_algorithm_module_thread_entry(monkeypatch):
    import threading
    import youth_wire
    fq = f"/youth_t_entry_{os.getpid()}"
    monkeypatch.setenv("YOUTH_ALGO_FRAME_QUEUE", fq)      # private queue, no pose queue
    monkeypatch.setenv("YOUTH_ALGO_POSE_QUEUE", "")
    lib = youth_icp.load_library()
    t = threading.Thread(target=lambda: lib.algorithmModule(None))
    t.start()
    for _ in range(200):
        if youth_icp.isSlamModuleRunning():
            break
        import time
        time.sleep(0.05)
    assert youth_icp.isSlamModuleRunning() == 1
    frames, _ = youth_synth.sequence(0, 2)
    assert youth_icp.processSlamFrame(frames[0], None, 640, 480, 0) == 1
    assert youth_icp.processSlamFrame(frames[1], None, 640, 480, 33) == 1
    assert youth_icp.slam_wait_idle(20000) == 1
    youth_icp.stopSlamModule()
    t.join(timeout=10)
    assert not t.is_alive()
    youth_wire.mq_unlink(fq)


# ------------------------------------------------ division path / alignment --
def test_projection_reciprocal_matches_ieee():
    """The projection reciprocal (icp_device.h proj_rcp_rn) equals IEEE
    1.0f / den bit for bit for EVERY fp32 den in its guarded range [2^-60,
    2^60] (exhaustive), and the projected pixel floor(fma(fx x', rz, cx) + 0.5)
    / in-range decision agrees with the IEEE reciprocal's on 2 x 2^30 random
    and near-half-integer cases, den inside and outside the guard."""
    for seed in (1, 0x5EED):
        bits, proj = youth_icp.selftest_projdiv(1 << 30, seed)
        assert bits == 0 and proj == 0, (seed, bits, proj)


def test_normal_normalisation_matches_ieee():
    """k_prep's fast normalisation (icp_device.h sqrt_rn_mid / norm_div)
    equals sqrtf and c / sqrtf(|c|^2) bit for bit: the sqrt exhaustively over
    [2^-96, 2^118], the quotients on 2 x 2^28 random vectors of mixed
    magnitude with signed zeros (most take the fast path)."""
    for seed in (1, 0x5EED):
        sq, quot, fast = youth_icp.selftest_normalize(1 << 28, seed)
        assert sq == 0 and quot == 0, (seed, sq, quot)
        assert fast > (1 << 27), fast


def test_fastdiv_path_is_bit_identical_to_ieee(monkeypatch):
    """The verified 3-op back-projection divide must change nothing: both
    paths give the same association and bit-identical poses."""
    src, dst, _ = youth_synth.pairs(30, 3)
    import torch
    ds = torch.from_numpy(src).cuda()
    dd = torch.from_numpy(dst).cuda()
    torch.cuda.synchronize()
    out = {}
    for mode in ("fast", "ieee"):
        if mode == "ieee":
            monkeypatch.setenv("YOUTH_ICP_NO_FASTDIV", "1")
        with youth_icp.IcpContext(640, 480, 3) as ctx:
            assert ctx.fastdiv == (mode == "fast")
            ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), 3)
            out[mode] = ctx.get_poses(3)[0]
            a, _ = ctx.reduce(src[0], dst[0], out[mode][0][:3].astype(np.float32))
            out[mode + "_assoc"] = a
    assert np.array_equal(out["fast"], out["ieee"])
    assert np.array_equal(out["fast_assoc"], out["ieee_assoc"])


def test_unaligned_source_pointer():
    """Source frames at an odd int16 offset take the unaligned depth path."""
    src, dst, _ = youth_synth.pairs(31, 2, 160, 120)
    import torch
    flat = torch.zeros(src.size + 1, dtype=torch.int16, device="cuda")
    flat[1:] = torch.from_numpy(src.reshape(-1)).cuda()
    dd = torch.from_numpy(dst).cuda()
    torch.cuda.synchronize()
    with youth_icp.IcpContext(160, 120, 2) as ctx:
        ctx.align_pairs_device(flat.data_ptr() + 2, dd.data_ptr(), 2)
        T64, _, st = ctx.get_poses(2)
    for p in range(2):
        To, _, sto, _ = oracle.align(src[p], dst[p])
        assert st[p] == sto and _pose_err(T64[p], To) <= POSE_TOL


def test_plain_c_host_demo(tmp_path):
    """The drop-in driven from plain C99 (pthread algorithmModule +
    processSlamFrame + saveSlamMap), as the reference's main.c would."""
    import subprocess
    from conftest import PKG
    exe = os.path.join(PKG, "slam_host_demo")
    base = str(tmp_path / "demo")
    r = subprocess.run([exe, os.path.join(GOLDEN, "astra_camera.yaml"), "6", base],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = np.loadtxt(base + "_trajectory.txt")
    assert rows.shape == (6, 8)
    frames, _ = youth_synth.sequence(0, 6)
    acc = np.eye(4)
    for k in range(1, 6):
        T64, _, _, _ = oracle.align(frames[k], frames[k - 1])
        acc = acc @ T64
    assert np.allclose(rows[-1, 1:4], acc[:3, 3], atol=1e-6)


def test_track_pipelined_copy_path(monkeypatch):
    """The tracker through the persistent kernel (YOUTH_ICP_NO_COOP=1): the
    result reaches the pinned slot by D2H copies and the frame's completion
    event keeps its system-scope fence (the cooperative path stores the result
    itself and records a fence-free event).  Two frames in flight equal
    track_frame bit for bit; every pose is the oracle's (<= 1e-5)."""
    monkeypatch.setenv("YOUTH_ICP_NO_COOP", "1")
    frames, _ = youth_synth.sequence(5, 6)
    with youth_icp.IcpContext(640, 480, 2) as ctx:
        want = [ctx.track_frame(f) for f in frames]
        assert ctx.get_plan()["kernel"] == PLAN["persistent"]
        ctx.track_reset()
        got = []
        for f in frames:
            ctx.track_submit(f)
            if ctx.track_pending() == 2:
                got.append(ctx.track_collect())
        while ctx.track_pending():
            got.append(ctx.track_collect())
    for (Tg, sg, hg), (Tw, sw, hw) in zip(got, want):
        assert np.array_equal(Tg, Tw) and sg == sw and hg == hw
    for k in range(1, len(frames)):
        T64, _, sto, _ = oracle.align(frames[k], frames[k - 1])
        assert got[k][2] and got[k][1] == sto and _pose_err(got[k][0], T64) <= POSE_TOL


PLAN = {"coop": "k_icp_coop", "persistent": "k_prep + k_icp (persistent)",
        "coop_refused": "k_prep + k_icp (persistent)",
        "per_iteration": "k_prep + k_init + k_reduce x iters (per-iteration)"}


@pytest.mark.parametrize("mode", ["coop", "persistent", "coop_refused", "per_iteration"])
def test_kernel_paths_match_oracle(monkeypatch, mode):
    """Every kernel path of an align gives the oracle's pose (<= 1e-5) and the
    oracle's per-iteration correspondence counts, on repeated calls: the
    small-batch cooperative kernel (k_icp_coop, fused prep); the persistent
    batch kernel (k_prep + k_icp); the persistent fallback taken when the
    runtime refuses the cooperative launch (forced by the
    YOUTH_ICP_TEST_REFUSE_COOP hook with the runtime launch path); and the
    per-iteration fallback (YOUTH_ICP_NO_PERSISTENT=1: k_reduce with the fused
    last-workgroup solve, once per iteration)."""
    if mode == "persistent":
        monkeypatch.setenv("YOUTH_ICP_NO_COOP", "1")
    if mode == "coop_refused":
        monkeypatch.setenv("YOUTH_ICP_COOP_LAUNCH", "runtime")
        monkeypatch.setenv("YOUTH_ICP_TEST_REFUSE_COOP", "1")
    if mode == "per_iteration":
        monkeypatch.setenv("YOUTH_ICP_NO_COOP", "1")
        monkeypatch.setenv("YOUTH_ICP_NO_PERSISTENT", "1")
    n = 3
    src, dst, _ = youth_synth.pairs(40, n)
    import torch
    ds = torch.from_numpy(src).cuda()
    dd = torch.from_numpy(dst).cuda()
    out = torch.zeros((n, 16), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with youth_icp.IcpContext(640, 480, n) as ctx:
        for _ in range(3):      # repeated calls: per-call state (counter sets, granules) re-armed
            ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), n, d_T_out=out.data_ptr())
        ctx.sync()
        plan = ctx.get_plan()
        T64, T32, st = ctx.get_poses(n)
        cnt, _ = ctx.get_stats(n, 10)
        lanes = lanes_of(ctx)
    assert plan["kernel"] == PLAN[mode]
    Tdev = out.cpu().numpy().reshape(n, 4, 4)
    for p in range(n):
        with oracle_like(lanes):
            T64o, _, sto, stats = oracle.align(src[p], dst[p], iters=10)
        assert st[p] == sto == 0
        assert _pose_err(T64[p], T64o) <= POSE_TOL
        assert np.array_equal(Tdev[p], T32[p])
        assert np.array_equal(cnt[p], stats[:, 0])


@pytest.mark.parametrize("mode", ["coop", "persistent"])
def test_kernel_paths_skipped_update(monkeypatch, mode):
    """A pair whose every iteration skips the update (no valid source pixels:
    YOUTH_STATUS_FEW_MATCHES) keeps its initial pose in T64, T32 and the fp32
    output on both kernel paths, while its batch neighbours converge."""
    if mode == "persistent":
        monkeypatch.setenv("YOUTH_ICP_NO_COOP", "1")
    n = 3
    src, dst, _ = youth_synth.pairs(50, n)
    src[1] = 0
    import torch
    ds = torch.from_numpy(src).cuda()
    dd = torch.from_numpy(dst).cuda()
    out = torch.full((n, 16), 7.0, dtype=torch.float32, device="cuda")
    T_init = np.tile(np.eye(4), (n, 1, 1))
    T_init[1, :3, 3] = [0.25, -0.5, 0.125]
    torch.cuda.synchronize()
    with youth_icp.IcpContext(640, 480, n) as ctx:
        ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), n, T_init=T_init,
                               d_T_out=out.data_ptr())
        ctx.sync()
        T64, T32, st = ctx.get_poses(n)
    Tdev = out.cpu().numpy().reshape(n, 4, 4)
    assert st[1] == youth_icp.STATUS_FEW_MATCHES
    assert np.array_equal(T64[1], T_init[1])
    assert np.array_equal(T32[1], T_init[1].astype(np.float32))
    assert np.array_equal(Tdev[1], T_init[1].astype(np.float32))
    for p in (0, 2):
        T64o, _, sto, _ = oracle.align(src[p], dst[p], iters=10, T_init=T_init[p])
        assert st[p] == sto == 0 and _pose_err(T64[p], T64o) <= POSE_TOL
        assert np.array_equal(Tdev[p], T32[p])


def test_non_finite_T_init_rejected():
    """T_init must be finite (the kernels' integer in-range test relies on
    finite projected coordinates): a NaN or inf entry is YOUTH_EINVAL before
    anything is enqueued, and the context keeps working."""
    import torch
    src, dst, _ = youth_synth.pairs(60, 2, 160, 120)
    ds, dd = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    torch.cuda.synchronize()
    with youth_icp.IcpContext(160, 120, 2) as ctx:
        for bad in (np.nan, np.inf):
            T_init = np.tile(np.eye(4), (2, 1, 1))
            T_init[1, 0, 3] = bad
            with pytest.raises(youth_icp.IcpError) as e:
                ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), 2, T_init=T_init)
            assert e.value.code == youth_icp.YOUTH_EINVAL
        ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), 2)
        ctx.sync()
        T64, _, st = ctx.get_poses(2)
    for p in range(2):
        To, _, sto, _ = oracle.align(src[p], dst[p])
        assert st[p] == sto and _pose_err(T64[p], To) <= POSE_TOL


def test_max_frame_size_8192x8192():
    """The largest frame youth_icp_create accepts (W*H = 2^26): 24-bit index
    multiply, 32-bit record byte offsets and the persistent path (one pair is
    too large for the cooperative kernel) at full size.  Pose within 1e-5 of
    the oracle; association at the final pose bit-exact over all 67 M pixels."""
    W = H = 8192
    K = youth_icp.default_intrinsics(W, H)
    src, dst, _ = youth_synth.pairs(7, 1, W, H)
    Tg, assoc = youth_icp.align_batch(src, dst, K=K, iters=2, want_assoc=True)
    T64, _, st, _ = oracle.align(src[0], dst[0], K, iters=2)
    assert st == 0 and _pose_err(Tg[0], T64) <= POSE_TOL
    idx = oracle.associate(src[0], dst[0], Tg[0][:3], K)
    assert int((idx >= 0).sum()) > W * H // 4
    assert np.array_equal(assoc[0], idx)


@pytest.mark.parametrize("W,H", [(16384, 48), (48, 16384)])
def test_extreme_aspect_frames(W, H):
    """The widest and the tallest frames youth_icp_create accepts with a
    short other side (W or H = 16384): 256 tiles across one row (or down one
    column), the 24-bit index multiply at its largest row stride, and partial
    tiles on the short side.  Two pairs in one batch and one pair per call
    (the cooperative kernel when its plan fits): poses within 1e-5 of the
    oracle, association at the final pose bit-exact."""
    import torch
    K = youth_icp.default_intrinsics(W, H)
    src, dst, _ = youth_synth.pairs(3, 2, W, H)
    Tg, assoc = youth_icp.align_batch(src, dst, K=K, want_assoc=True)
    for p in range(2):
        To, _, st, _ = oracle.align(src[p], dst[p], K)
        assert st == 0 and _pose_err(Tg[p], To) <= POSE_TOL, p
        idx = oracle.associate(src[p], dst[p], Tg[p][:3], K)
        assert int((idx >= 0).sum()) > W * H // 8
        assert np.array_equal(assoc[p], idx), p
    ctx = youth_icp.IcpContext(W, H, 2, K=K)
    ds, dd = torch.from_numpy(src[:1]).cuda(), torch.from_numpy(dst[:1]).cuda()
    ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), 1)
    T64, _, st = ctx.get_poses(1)
    plan = ctx.get_plan()
    ctx.close()
    To, _, sto, _ = oracle.align(src[0], dst[0], K)
    assert st[0] == sto == 0 and _pose_err(T64[0], To) <= POSE_TOL, plan


def test_plain_c_batch_multi_demo(tmp_path):
    """youth_icp_align_batch_multi driven from plain C99 over every visible
    device (examples/batch_multi_demo.c): every pose within 1e-5 of the
    oracle."""
    import subprocess
    from conftest import PKG
    n, W, H = 6, 320, 240
    out = str(tmp_path / "T.f32")
    r = subprocess.run([os.path.join(PKG, "batch_multi_demo"), str(n), out, str(W), str(H)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    T = np.fromfile(out, np.float32).reshape(n, 4, 4)
    src, dst, _ = youth_synth.pairs(0, n, W, H)
    T_cpu, st = oracle.align_batch(src, dst, iters=10, n_threads=min(n, os.cpu_count() or 1))
    assert not st.any()
    for p in range(n):
        assert _pose_err(T[p], T_cpu[p]) <= POSE_TOL, p


def test_rccl_pose_gather_c_abi_one_rank():
    """youth_dist.h through RCCL on this box's GPU at N = 1 (the
    multi-process form needs one GPU per rank; N > 1 is the driver's 8-GPU
    run): the device and host gathers return every row in pair order."""
    import torch
    import youth_dist
    g = youth_dist.RcclPoseGather(1, 0, 0, youth_dist.unique_id())
    try:
        rng = np.random.default_rng(5)
        for n in (1, 37, 512):
            loc = rng.standard_normal((n, 16)).astype(np.float32)
            assert np.array_equal(g.allgather_host(loc, n), loc)
            d_loc = torch.from_numpy(loc).cuda()
            d_all = torch.zeros_like(d_loc)
            s = torch.cuda.current_stream()
            g.allgather_device(d_loc.data_ptr(), n, d_all.data_ptr(), s.cuda_stream)
            torch.cuda.synchronize()
            assert torch.equal(d_all, d_loc)
    finally:
        g.close()


def test_plain_c_rccl_demo_one_rank(tmp_path):
    """examples/batch_rccl_demo.c (one process per GPU: shard align +
    youth_dist_allgather_poses_host) as rank 0 of 1: id file bootstrap, the
    gathered poses within 1e-5 of the oracle."""
    import subprocess
    from conftest import PKG
    n, W, H = 4, 320, 240
    out = str(tmp_path / "T.f32")
    r = subprocess.run([os.path.join(PKG, "batch_rccl_demo"), "1", "0", str(tmp_path / "id"),
                        str(n), out, str(W), str(H)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    T = np.fromfile(out, np.float32).reshape(n, 4, 4)
    src, dst, _ = youth_synth.pairs(0, n, W, H)
    T_cpu, st = oracle.align_batch(src, dst, iters=10, n_threads=min(n, os.cpu_count() or 1))
    assert not st.any()
    for p in range(n):
        assert _pose_err(T[p], T_cpu[p]) <= POSE_TOL, p


def test_headline_512_pairs_one_launch():
    """C4 at N = 1, exactly as bench.py's `value` runs it: 512 pairs @640x480
    in ONE align_pairs_device call, i.e. the persistent k_icp with the
    >256-pair work geometry (3072 chunks per iteration, 6 per pair;
    reduce_geometry).  Every one of the 512 poses within 1e-5 of the oracle's;
    the correspondence count of every pair at every iteration equal to the
    oracle's (the association inside k_icp, which emits no indices, picks the
    same pixel set) and sum r^2 within rel 1e-9; indices at the final fp32
    pose bit-exact on pairs 0, 255, 256 and 511 (first/last pair of each half
    of the batch, the 8-GPU shard boundaries 256 apart)."""
    import torch
    n, W, H = 512, 640, 480
    src, dst, _ = youth_synth.pairs(0, n, W, H)
    ds = torch.from_numpy(src).cuda()
    dd = torch.from_numpy(dst).cuda()
    out = torch.zeros((n, 16), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with youth_icp.IcpContext(W, H, n, iters=10) as ctx:
        ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), n, d_T_out=out.data_ptr())
        ctx.sync()
        assert ctx.get_plan()["kernel"].startswith("k_prep + k_icp (persistent)")
        T64, T32, st = ctx.get_poses(n)
        cnt, r2 = ctx.get_stats(n, 10)
        Tout = out.cpu().numpy().reshape(n, 4, 4)
        lanes = lanes_of(ctx)
    del ds, dd
    with oracle_like(lanes):
        T_cpu, st_cpu, stats = oracle.align_batch(src, dst, iters=10,
                                                  n_threads=min(16, os.cpu_count() or 1),
                                                  want_stats=True)
    assert not st.any() and not st_cpu.any()
    err = np.abs(T64[:, :3, :4] - T_cpu[:, :3, :4]).max(axis=(1, 2))
    assert float(err.max()) <= POSE_TOL, (int(err.argmax()), float(err.max()))
    assert np.array_equal(Tout, T32)
    assert np.array_equal(cnt, stats[..., 0]), np.argwhere(cnt != stats[..., 0])[:4]
    # sum r^2 of an iteration: fp64 summation order, and the fp32 pose of the
    # iteration is (float)T64, which can land one ulp apart when T64 differs
    # in its last bits next to an fp32 rounding boundary (seen once in 5120
    # pair-iterations: rel 1.3e-9)
    np.testing.assert_allclose(r2, stats[..., 1], rtol=1e-6)
    K = oracle.viewer_K(W, H)
    with youth_icp.IcpContext(W, H, 2) as ctx:
        for p in (0, 255, 256, 511):
            g_idx, _ = ctx.reduce(src[p], dst[p], T32[p][:3])
            assert np.array_equal(g_idx, oracle.associate(src[p], dst[p], T32[p][:3], K)), p


def test_concurrent_contexts_share_the_device():
    """youth_icp_set_concurrency(2) on two contexts whose persistent aligns
    run side by side on two streams (bench.py's small shards, N = 8's 64
    pairs): each k_icp on half the workgroup slots with half the chunks.
    Both batches of 64 pairs @640x480, aligned twice in interleaved order,
    within 1e-5 of the oracle with every pair's correspondence count at every
    iteration equal to the oracle's, and the repeat bit-identical to the
    first.  Out-of-range shares are refused and the setter returns the
    previous value."""
    import torch
    n, W, H = 64, 640, 480
    batches = [youth_synth.pairs(seed, n, W, H)[:2] for seed in (5, 6)]
    dev = [(torch.from_numpy(s).cuda(), torch.from_numpy(d).cuda()) for s, d in batches]
    outs = [torch.zeros((n, 16), dtype=torch.float32, device="cuda") for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    torch.cuda.synchronize()
    ctxs = [youth_icp.IcpContext(W, H, n, iters=10) for _ in range(2)]
    lanes = [None, None]
    try:
        for c in ctxs:
            with pytest.raises(youth_icp.IcpError):
                c.set_concurrency(0)
            with pytest.raises(youth_icp.IcpError):
                c.set_concurrency(youth_icp.MAX_CONCURRENCY + 1)
            assert c.set_concurrency(2) == 1
        got = []
        for rep in range(2):
            for q in range(2):
                ctxs[q].align_pairs_device(dev[q][0].data_ptr(), dev[q][1].data_ptr(), n,
                                           d_T_out=outs[q].data_ptr(),
                                           stream=streams[q].cuda_stream)
            res = []
            for q in range(2):
                ctxs[q].sync(streams[q].cuda_stream)
                assert ctxs[q].get_plan()["kernel"].startswith("k_prep + k_icp (persistent)")
                T64, T32, st = ctxs[q].get_poses(n)
                cnt, _ = ctxs[q].get_stats(n, 10)
                assert np.array_equal(outs[q].cpu().numpy().reshape(n, 4, 4), T32)
                res.append((T64, st, cnt))
                lanes[q] = lanes_of(ctxs[q])
            got.append(res)
        assert ctxs[0].set_concurrency(1) == 2
    finally:
        for c in ctxs:
            c.close()
    for q, (src, dst) in enumerate(batches):
        with oracle_like(lanes[q]):
            T_cpu, st_cpu, stats = oracle.align_batch(src, dst, iters=10,
                                                      n_threads=min(16, os.cpu_count() or 1),
                                                      want_stats=True)
        T64, st, cnt = got[0][q]
        assert not st.any() and not st_cpu.any()
        err = np.abs(T64[:, :3, :4] - T_cpu[:, :3, :4]).max()
        assert float(err) <= POSE_TOL, (q, float(err))
        assert np.array_equal(cnt, stats[..., 0]), (q, np.argwhere(cnt != stats[..., 0])[:4])
        for a, b in zip(got[0][q], got[1][q]):
            assert np.array_equal(a, b), q


@pytest.mark.parametrize("xcd_map", ["1", "2"])
def test_prep_tile_orders_bit_identical(xcd_map, monkeypatch):
    """k_prep's workgroup -> tile orders (YOUTH_ICP_PREP_XCD_MAP: 0 row-major
    over the frames, 1 one contiguous run per XCD, 2 tile rows dealt over the
    XCDs with a padded grid) only reorder the tiles: records and the aligned
    poses equal the default order's bit for bit, frames whose tile-row count
    is not a multiple of 8 included (97x53: 2 x 2 tiles)."""
    import torch
    for W, H, n in ((640, 480, 12), (97, 53, 5)):
        src, dst, _ = youth_synth.pairs(40, n, W, H)
        ds, dd = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
        torch.cuda.synchronize()
        out = {}
        for m in ("0", xcd_map):
            monkeypatch.setenv("YOUTH_ICP_PREP_XCD_MAP", m)
            monkeypatch.setenv("YOUTH_ICP_NO_COOP", "1")
            with youth_icp.IcpContext(W, H, n) as ctx:
                rec = ctx.prepare(dst, want_normals=True, want_xyz=False)
                ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), n)
                T64, _, st = ctx.get_poses(n)
            out[m] = (rec, T64, st)
        for a, b in zip(out["0"][0][3:], out[xcd_map][0][3:]):
            assert np.array_equal(_bits(a), _bits(b))
        assert np.array_equal(out["0"][1], out[xcd_map][1])
        assert np.array_equal(out["0"][2], out[xcd_map][2]) and not out["0"][2].any()


def test_track_micro_batches_bit_identical():
    """youth_icp_track_submit_batch: two consecutive frames aligned by ONE
    k_icp_coop launch (pair 1 waits for pair 0's prep of its target), each
    frame collected separately with exactly the result track_frame gives in
    the same mode (pose bits, status, has_ref): the first frame of a
    sequence, odd counts, singles between batches, a reset with a batch in
    flight, the library loop in micro-batches; the default plan (one pair
    per grid: per-frame launches) and the batch mode's plan (5 px per lane:
    chained launches), both within 1e-5 of the oracle; a context too small
    for batches falls back to per-frame launches."""
    frames, _ = youth_synth.sequence(5, 12)
    for batch_mode, max_frames in ((False, 4), (True, 4), (True, 2)):
        with youth_icp.IcpContext(640, 480, 4) as ref:
            if batch_mode:
                ref.track_set_batch(2)
            want = [ref.track_frame(f) for f in frames]
        for k in range(1, len(frames)):
            T64, _, sto, _ = oracle.align(frames[k], frames[k - 1])
            assert want[k][1] == sto and _pose_err(want[k][0], T64) <= POSE_TOL
        with youth_icp.IcpContext(640, 480, max_frames) as ctx:
            if batch_mode:
                ctx.track_set_batch(2)
            got = []
            ctx.track_submit_batch(frames[0:2])            # no reference: prep + one align
            got += [ctx.track_collect() for _ in range(2)]
            ctx.track_submit_batch(frames[2:4])            # one chained launch
            ctx.track_submit(frames[4])                    # a single behind it
            got += [ctx.track_collect() for _ in range(3)]
            for k in range(5, 11, 2):
                ctx.track_submit_batch(frames[k:k + 2])
                got.append(ctx.track_collect())
                got.append(ctx.track_collect())
            ctx.track_submit_batch(frames[11:12])          # a batch of one
            got.append(ctx.track_collect())
            chained = ctx.track_chained()
            assert chained == (4 if batch_mode and max_frames >= 4 else 0), chained
            assert ctx.track_pending() == 0 and len(got) == len(want)
            for k, ((Tg, sg, hg), (Tw, sw, hw)) in enumerate(zip(got, want)):
                assert np.array_equal(Tg, Tw) and sg == sw and hg == hw, (batch_mode, k)
            with pytest.raises(youth_icp.IcpError):
                ctx.track_submit_batch(frames[0:youth_icp.TRACK_MAX_BATCH + 1])
            ctx.track_reset()
            ctx.track_submit_batch(frames[0:2])
            ctx.track_reset()                              # batch in flight
            ctx.track_submit(frames[3])
            hs = [ctx.track_collect()[2] for _ in range(3)]
            assert hs == [False, True, False]
            ctx.track_reset()
            Tb, stb = ctx.track_host_sequence(frames)
            assert np.array_equal(Tb, np.stack([w[0] for w in want[1:]]))
            assert np.array_equal(stb, np.array([w[1] for w in want[1:]], np.int32))


def test_coop_launches_from_several_streams():
    """Cooperative launches from three contexts at once, issued interleaved
    from one host thread without syncs: two single-pair aligns on two torch
    streams and a tracker in micro-batches of two on its own stream.  The
    library orders a device's k_icp_coop grids across streams (coop_enqueue),
    so none waits on a workgroup that cannot be resident: no timeout, and
    every result equals the one each context gives alone, bit for bit."""
    import torch
    N = 640 * 480
    src, dst, _ = youth_synth.pairs(40, 2)
    frames, _ = youth_synth.sequence(21, 9)
    ds, dd = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    torch.cuda.synchronize()
    want = []
    for p in range(2):
        with youth_icp.IcpContext(640, 480, 2) as ctx:
            ctx.align_pairs_device(ds.data_ptr() + 2 * N * p, dd.data_ptr() + 2 * N * p, 1)
            want.append(ctx.get_poses(1)[1][0])
    with youth_icp.IcpContext(640, 480, 4) as ref:
        ref.track_set_batch(2)
        want_trk = [ref.track_frame(f) for f in frames]
    reps = 24
    outs = [torch.zeros((reps, 16), device="cuda") for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    ctxs = [youth_icp.IcpContext(640, 480, 2) for _ in range(2)]
    trk = youth_icp.IcpContext(640, 480, 4)
    trk.track_set_batch(2)
    got_trk = []
    try:
        trk.track_submit(frames[0])
        f = 1
        for r in range(reps):
            for p in range(2):
                ctxs[p].align_pairs_device(ds.data_ptr() + 2 * N * p, dd.data_ptr() + 2 * N * p,
                                           1, d_T_out=outs[p][r].data_ptr(),
                                           stream=streams[p].cuda_stream)
            if f + 2 <= len(frames) and r % 3 == 0:
                trk.track_submit_batch(frames[f:f + 2])
                f += 2
            while trk.track_pending() > 2:
                got_trk.append(trk.track_collect())
        while trk.track_pending():
            got_trk.append(trk.track_collect())
        torch.cuda.synchronize()
        for p in range(2):
            assert not ctxs[p].get_poses(1)[2].any()
            rows = outs[p].cpu().numpy().reshape(reps, 4, 4)
            for r in range(reps):
                assert np.array_equal(rows[r][:3], want[p][:3]), (p, r)
    finally:
        for c in ctxs + [trk]:
            c.close()
    assert len(got_trk) == f
    for (Tg, sg, hg), (Tw, sw, hw) in zip(got_trk, want_trk):
        assert np.array_equal(Tg, Tw) and sg == sw and hg == hw


def test_coop_launches_from_host_threads():
    """Four host threads, each with its own context and stream, align single
    pairs concurrently (ctypes drops the GIL inside the library): the device's
    cooperative launches are ordered under its lock from every thread, and
    every thread gets the pose its pair gives alone, bit for bit."""
    import threading
    import torch
    src, dst, _ = youth_synth.pairs(60, 4)
    ds, dd = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    torch.cuda.synchronize()
    N = 640 * 480

    def align(ctx, p, stream):
        ctx.align_pairs_device(ds.data_ptr() + 2 * N * p, dd.data_ptr() + 2 * N * p, 1,
                               stream=stream.cuda_stream)
        stream.synchronize()
        T64, _, st = ctx.get_poses(1)
        return T64[0], int(st[0])

    want = []
    s0 = torch.cuda.Stream()
    for p in range(4):
        with youth_icp.IcpContext(640, 480, 2) as ctx:
            want.append(align(ctx, p, s0))
    errors, results = [], [None] * 4

    def worker(p):
        try:
            stream = torch.cuda.Stream()
            with youth_icp.IcpContext(640, 480, 2) as ctx:
                results[p] = [align(ctx, p, stream) for _ in range(12)]
        except Exception as e:  # reported by the main thread
            errors.append(f"{p}: {e!r}")

    threads = [threading.Thread(target=worker, args=(p,)) for p in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads) and not errors, errors
    for p in range(4):
        assert want[p][1] == 0 and len(results[p]) == 12
        for T, st in results[p]:
            assert st == 0 and np.array_equal(T, want[p][0]), p


def test_track_micro_batches_1280x960():
    """C3's frame size through the tracker in micro-batches of two (the plan
    whose two grids fit the chip: 20 px per lane, 120 workgroups per pair,
    123 KB of source LDS per workgroup): every frame bit-identical to
    track_frame in the same plan, chained launches used, and within 1e-5 of
    the oracle at 20 iterations."""
    W, H, it = 1280, 960, 20
    frames, _ = youth_synth.sequence(3, 7, W, H)
    K = youth_icp.default_intrinsics(W, H)
    with youth_icp.IcpContext(W, H, 4, K=K, iters=it) as ref:
        ref.track_set_batch(2)
        want = [ref.track_frame(f) for f in frames]
        plan = ref.get_plan()
    with youth_icp.IcpContext(W, H, 4, K=K, iters=it) as ctx:
        ctx.track_set_batch(2)
        Tb, stb = ctx.track_host_sequence(frames)
        chained = ctx.track_chained()
    assert chained >= 2, (chained, plan)
    assert np.array_equal(Tb, np.stack([w[0] for w in want[1:]]))
    assert np.array_equal(stb, np.array([w[1] for w in want[1:]], np.int32))
    for k in (1, len(frames) - 1):
        T64, _, sto, _ = oracle.align(frames[k], frames[k - 1], iters=it)
        assert want[k][1] == sto and _pose_err(want[k][0], T64) <= POSE_TOL


@pytest.mark.parametrize("spec", ["survey", "fma"])
@pytest.mark.parametrize("W,H", [(97, 53), (160, 120)])
def test_track_micro_batches_ragged_sizes(W, H, spec):
    """Micro-batches of 4 at ragged frame sizes (narrow halo loads, partial
    tiles, a few workgroups per pair) in both arithmetics: the library loop
    bit-identical to track_frame in the same plan, every frame within 1e-5
    of the oracle in that arithmetic."""
    oracle.set_spec(spec)
    try:
        frames, _ = youth_synth.sequence(11, 9, W, H)
        K = youth_icp.default_intrinsics(W, H)
        with youth_icp.IcpContext(W, H, 8, K=K, spec=spec) as ref:
            ref.track_set_batch(4)
            want = [ref.track_frame(f) for f in frames]
        with youth_icp.IcpContext(W, H, 8, K=K, spec=spec) as ctx:
            ctx.track_set_batch(4)
            Tb, stb = ctx.track_host_sequence(frames)
            assert ctx.track_chained() >= 2
        assert np.array_equal(Tb, np.stack([w[0] for w in want[1:]]))
        assert np.array_equal(stb, np.array([w[1] for w in want[1:]], np.int32))
        for k in range(1, len(frames)):
            T64, _, sto, _ = oracle.align(frames[k], frames[k - 1])
            assert want[k][1] == sto and _pose_err(want[k][0], T64) <= POSE_TOL, k
    finally:
        oracle.set_spec("survey")


@pytest.mark.parametrize("batch", [3, 4])
def test_track_micro_batches_up_to_four(batch):
    """Micro-batches of up to TRACK_MAX_BATCH frames (youth_icp_track_set_batch(
    batch): the plan whose `batch` grids fit the chip at once less the 32 CUs
    kept free for the next micro-batch's k_pull_frames, 9 / 11 px per lane at
    640x480): chains of 4, 3 and 2 frames, a submission longer than
    the plan holds split into the longest chains that fit, and the library
    loop with two submissions in flight, every frame bit-identical to
    track_frame in the same plan and within 1e-5 of the oracle."""
    frames, _ = youth_synth.sequence(7, 14)
    with youth_icp.IcpContext(640, 480, 8) as ref:
        ref.track_set_batch(batch)
        want = [ref.track_frame(f) for f in frames]
        plan = ref.get_plan()
    assert plan["px_per_lane"] == {3: 9, 4: 11}[batch]
    for k in range(1, len(frames)):
        T64, _, sto, _ = oracle.align(frames[k], frames[k - 1])
        assert want[k][1] == sto and _pose_err(want[k][0], T64) <= POSE_TOL
    with youth_icp.IcpContext(640, 480, 2 * batch) as ctx:
        ctx.track_set_batch(batch)
        got = []
        ctx.track_submit(frames[0])                        # the reference
        k = 1
        for m in (4, 3, 2, 1, 3):
            ctx.track_submit_batch(frames[k:k + m])
            got += [ctx.track_collect() for _ in range(m)]
            k += m
        while ctx.track_pending():
            got.append(ctx.track_collect())
        assert len(got) == len(frames)
        # chains: 4 (batch 3: a chain of 3 + one frame); 3; 2; none; 3
        assert ctx.track_chained() == 4, ctx.track_chained()
        for bad in (0, youth_icp.TRACK_MAX_BATCH + 1):
            with pytest.raises(youth_icp.IcpError):
                ctx.track_set_batch(bad)
            with pytest.raises(youth_icp.IcpError):
                ctx.track_submit_batch(frames[:bad] if bad else frames[:0])
        for i, ((Tg, sg, hg), (Tw, sw, hw)) in enumerate(zip(got, want)):
            assert np.array_equal(Tg, Tw) and sg == sw and hg == hw, (batch, i)
        ctx.track_reset()
        Tb, stb = ctx.track_host_sequence(frames)
        assert np.array_equal(Tb, np.stack([w[0] for w in want[1:]]))
        assert np.array_equal(stb, np.array([w[1] for w in want[1:]], np.int32))


@pytest.mark.parametrize("W,H", [(640, 480), (97, 53)])
def test_track_frame_copy_paths_bit_identical(monkeypatch, W, H):
    """The tracker's H2D of host frames: k_pull_frames (the default: the GPU
    pulls the page-locked frames itself, 16-byte body when both ends are
    aligned, element tail; 97x53 frames are 10,282 bytes, so every other
    device slot is misaligned and takes the element path) against the SDMA
    copy engine (YOUTH_ICP_TRACK_COPY=sdma): the same poses bit for bit, one
    frame per launch and in micro-batches of 4, through track_host_sequence
    (staged copies) and track_submit_pinned (the caller's page-locked
    buffers).  Also the staging copy of a micro-batch (2.4 MB at 640x480)
    split over helper threads (the default) against one thread
    (YOUTH_ICP_COPY_THREADS=0)."""
    frames, _ = youth_synth.sequence(17, 9, W, H)
    K = youth_icp.default_intrinsics(W, H)
    res = {}
    for path in ("sdma", "pull", "pull_1thread"):
        if path == "sdma":
            monkeypatch.setenv("YOUTH_ICP_TRACK_COPY", "sdma")
        else:
            monkeypatch.delenv("YOUTH_ICP_TRACK_COPY", raising=False)
        if path == "pull_1thread":
            monkeypatch.setenv("YOUTH_ICP_COPY_THREADS", "0")
        else:
            monkeypatch.delenv("YOUTH_ICP_COPY_THREADS", raising=False)
        out = []
        for batch in (1, 4):
            with youth_icp.IcpContext(W, H, 8, K=K) as ctx:
                if batch > 1:
                    ctx.track_set_batch(batch)
                out.append(ctx.track_host_sequence(frames)[0])
                ctx.track_reset()
                bufs = [youth_icp.PinnedFrame(H, W) for _ in frames]
                for b, f in zip(bufs, frames):
                    b.array[:] = f
                got = []
                for i in range(0, len(bufs), batch):
                    ctx.track_submit_pinned(bufs[i:i + batch])
                    while ctx.track_pending():
                        T, _, has = ctx.track_collect()
                        if has:
                            got.append(T)
                out.append(np.stack(got))
                for b in bufs:
                    b.close()
        res[path] = out
    for other in ("sdma", "pull_1thread"):
        for a, b in zip(res[other], res["pull"]):
            assert np.array_equal(a, b), other
    T64, _, _, _ = oracle.align(frames[1], frames[0])
    assert _pose_err(res["pull"][0][0], T64) <= POSE_TOL


def test_track_submit_pinned_pageable_buffers_fall_back():
    """youth_icp_track_submit_pinned with buffers youth_icp_host_alloc did not
    make (pageable numpy arrays, a contract violation): the GPU must not read
    them in place (that would fault); the submission takes hipMemcpyAsync and
    the poses equal those from page-locked buffers bit for bit."""
    import ctypes

    class NumpyFrame:
        def __init__(self, a):
            self.array = np.ascontiguousarray(a)
            self.ptr = self.array.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))

    frames, _ = youth_synth.sequence(19, 5)
    out = []
    for make in (lambda f: NumpyFrame(f), None):
        with youth_icp.IcpContext(640, 480, 8) as ctx:
            ctx.track_set_batch(4)
            if make is None:
                bufs = [youth_icp.PinnedFrame(480, 640) for _ in frames]
                for b, f in zip(bufs, frames):
                    b.array[:] = f
            else:
                bufs = [make(f) for f in frames]
            got = []
            ctx.track_submit_pinned(bufs[:1])
            ctx.track_submit_pinned(bufs[1:])
            while ctx.track_pending():
                T, _, has = ctx.track_collect()
                if has:
                    got.append(T)
            out.append(np.stack(got))
            if make is None:
                for b in bufs:
                    b.close()
    assert np.array_equal(out[0], out[1])


@pytest.mark.parametrize("iters", [1, 2, 3, 10])
def test_coop_partial_rows_reused_across_call_sizes(iters):
    """k_icp_coop's counter-free hand-off: every partial row is EMPTY before
    it is stored, rows are triple-buffered by iteration and alternate between
    two arenas by call, each call resetting the rows the previous one used.
    Calls of 1, 8, 3 and 5 pairs (grids of different rows per buffer), in an
    interleaved order on ONE context, with 1-3 iterations (the reset of buffer
    (k+2) % 3 skipped or not) and 10: every result bit-identical to the same
    call on a fresh context, no timeout, and the 1-pair pose within the bar
    of the oracle."""
    import torch
    N = 640 * 480
    src, dst, _ = youth_synth.pairs(52, 8)
    ds, dd = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    sizes = (1, 8, 3, 5)
    want = {}
    for n in sizes:
        with youth_icp.IcpContext(640, 480, 16, iters=iters) as ctx:
            ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), n)
            assert ctx.get_plan()["kernel"] == "k_icp_coop"
            T64, _, st = ctx.get_poses(n)
            assert not st.any()
            want[n] = T64.copy()
    with youth_icp.IcpContext(640, 480, 16, iters=iters) as ctx:
        for n in (8, 1, 5, 1, 3, 8, 3, 1, 5, 5, 8, 1):
            ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), n)
            T64, _, st = ctx.get_poses(n)
            assert not st.any(), (n, st)
            assert np.array_equal(T64, want[n]), n
    To, _, sto, _ = oracle.align(src[0], dst[0], iters=iters)
    assert sto == 0 and _pose_err(want[1][0], To) <= POSE_TOL


def test_coop_lost_row_times_out_and_context_recovers(monkeypatch):
    """A k_icp_coop launch in which one workgroup never stores its partial
    row (test hook YOUTH_ICP_TEST_COOP_STALL: chunk 7 of pair 0 skips
    iteration 1's row; the hook's waits give up after 20000 polls) ends with
    YOUTH_STATUS_TIMEOUT instead of hanging, and leaves its arena part EMPTY
    and part written: the same context's next calls (on the other arena,
    then on the reset one) give every pose bit-identical to a fresh
    context's."""
    import torch
    src, dst, _ = youth_synth.pairs(53, 3)
    ds, dd = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    want = {}
    for n in (1, 3):
        with youth_icp.IcpContext(640, 480, 4) as ctx:
            ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), n)
            want[n] = ctx.get_poses(n)[0].copy()
    monkeypatch.setenv("YOUTH_ICP_TEST_COOP_STALL", "7")
    with youth_icp.IcpContext(640, 480, 4) as ctx:
        ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), 1)
        assert ctx.get_plan()["kernel"] == "k_icp_coop"
        st = ctx.get_poses(1)[2]
        assert st[0] & youth_icp.STATUS_TIMEOUT, st
        for n in (3, 1, 3):
            ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), n)
            T64, _, st = ctx.get_poses(n)
            assert not st.any(), (n, st)
            assert np.array_equal(T64, want[n]), n


@pytest.mark.parametrize("W,H", [(640, 480), (320, 240), (160, 120), (97, 53)])
def test_coop_polled_rows_back_to_back(W, H):
    """k_icp_coop's polled partial rows under load: 600 single-pair aligns
    back to back on one stream (two arenas alternating, rows reset by the
    next-but-one call, every iteration's wait on rows that are still landing),
    every fp32 pose bit-identical to the first and no timeout."""
    import torch
    K = youth_icp.default_intrinsics(W, H)
    src, dst, _ = youth_synth.pairs(61, 1, W, H)
    ds, dd = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    reps = 600
    out = torch.zeros((reps, 16), device="cuda")
    with youth_icp.IcpContext(W, H, 2, K=K) as ctx:
        for r in range(reps):
            ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), 1, d_T_out=out[r].data_ptr())
        torch.cuda.synchronize()
        assert ctx.get_plan()["kernel"] == "k_icp_coop"
        assert not ctx.get_poses(1)[2].any()
    rows = out.cpu().numpy()
    assert (rows == rows[0]).all()
