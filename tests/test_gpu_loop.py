"""Loop closing on the GPU (include/youth_loop.h): the signature
and distance kernels bit for bit against tests/loop_truth.py (the distance
also on made-up records at 20 x 15, where a pixel is a cell), the candidate
order, and the verification of the C5 revisit (frame 630 sees what frame 0
saw) against the numpy RGB-D alignment and the ground truth."""
import numpy as np
import pytest
import torch

import loop_truth
import rgbd_truth
import youth_icp
import youth_loop
import youth_synth

pytestmark = pytest.mark.gpu

K160 = (142.575, 142.575, 80.0, 60.0, 1000.0)


# ------------------------------------------------------------------ signature --
def _frames(n, W, H, seed):
    """n frames with holes, negative depths and (from the second on) one
    all-zero frame; intensities random."""
    rng = np.random.default_rng(seed)
    d = rng.integers(300, 6000, (n, H, W)).astype(np.int16)
    d[rng.random((n, H, W)) < 0.25] = 0
    d[rng.random((n, H, W)) < 0.05] = -7
    # whole cells without depth, and cells around the 4 cnt >= n threshold
    d[:, : H // 3, : W // 4] = 0
    keep = rng.random((n, H, W)) < 0.25
    d[:, H // 2:, W // 2:] = np.where(keep, 1234, 0)[:, H // 2:, W // 2:]
    if n > 1:
        d[1] = 0
    y = rng.integers(0, 256, (n, H, W)).astype(np.uint8)
    return d, y


def _gpu_signature(d, y, offset=0):
    """The kernel on device copies; offset > 0 places both planes that many
    bytes off a 16-byte boundary (the scalar-load path)."""
    n, H, W = d.shape
    td = torch.zeros(d.size + 8 + offset, dtype=torch.int16, device="cuda")
    ty = torch.zeros(y.size + 16 + offset, dtype=torch.uint8, device="cuda")
    od, oy = offset // 2 if offset else 0, offset
    td[od:od + d.size] = torch.from_numpy(d.ravel()).cuda()
    ty[oy:oy + y.size] = torch.from_numpy(y.ravel()).cuda()
    sig = torch.full((n, 300), 0xDEAD, dtype=torch.int32, device="cuda")
    youth_loop.signature_device(td.data_ptr() + 2 * od, ty.data_ptr() + oy, n, W, H, sig.data_ptr())
    torch.cuda.synchronize()
    return sig.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("W,H,n", [(20, 15, 1), (23, 17, 5), (97, 53, 5), (80, 60, 5), (160, 120, 1),
                                   (160, 120, 5), (640, 480, 2), (4112, 15, 1)],
                         ids=lambda v: str(v))
def test_signature_is_bit_exact(W, H, n):
    """One pixel per cell, ragged cells, cells of 4 and 8 pixels inside 16-pixel
    loads, whole-unit cells (640), a row wider than a workgroup's 256 units."""
    d, y = _frames(n, W, H, 100 + W)
    want = np.array([loop_truth.signature(d[k], y[k]) for k in range(n)])
    got = _gpu_signature(d, y)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    if n > 1:
        assert (want[1] >> 31 == 0).all() and (want[0] >> 31).any() and not (want[0] >> 31).all()


@pytest.mark.parametrize("W,H", [(160, 120), (640, 480)], ids=lambda v: str(v))
def test_signature_does_not_depend_on_the_load_width(W, H):
    d, y = _frames(2, W, H, 7)
    want = np.array([loop_truth.signature(d[k], y[k]) for k in range(2)])
    assert np.array_equal(_gpu_signature(d, y, offset=2), want)


def test_signature_sums_past_32_bits():
    """7680 x 5400 of depth 32767: cells of 384 x 360 pixels sum to 4.53e9."""
    W, H = 7680, 5400
    d = np.full((1, H, W), 32767, np.int16)
    y = np.random.default_rng(3).integers(0, 256, (1, H, W)).astype(np.uint8)
    d[0, :360, :384] = 0          # cell 0 invalid
    d[0, :360, 384:768:2] = 0     # cell 1 half valid: still 32767
    assert 384 * 360 * 32767 > 2 ** 32
    want = loop_truth.signature(d[0], y[0])
    assert want[0] >> 31 == 0 and (want[1] & 0xFFFF) == 32767 and (want[2] & 0xFFFF) == 32767
    got = _gpu_signature(d, y)
    assert np.array_equal(got[0], want), np.argwhere(got[0] != want)[:5]


def test_signature_argument_errors():
    t = torch.zeros(64 * 64, dtype=torch.int16, device="cuda")
    g = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
    s = torch.zeros(300, dtype=torch.int32, device="cuda")
    for W, H in ((19, 15), (20, 14)):
        with pytest.raises(youth_icp.IcpError) as ei:
            youth_loop.signature_device(t.data_ptr(), g.data_ptr(), 1, W, H, s.data_ptr())
        assert ei.value.code == youth_icp.YOUTH_EINVAL
    with pytest.raises(youth_icp.IcpError):
        youth_loop.signature_device(0, g.data_ptr(), 1, 20, 15, s.data_ptr())
    with pytest.raises(youth_icp.IcpError):
        youth_loop.LoopCloser(19, 15)
    with pytest.raises(youth_icp.IcpError):
        youth_loop.LoopCloser(160, 120, max_keyframes=513)
    with pytest.raises(youth_icp.IcpError):
        youth_loop.LoopCloser(160, 120, max_candidates=17)


# ------------------------------------------- k_loop_distance on made-up records --
# At 20 x 15 one pixel is one cell, so the stored record of a keyframe is
# depth | gray << 16 | (depth > 0) << 31 (depth <= 0: gray << 16) and
# add_keyframe_device stores any signature one likes.
N_STORE, N_QUERY = 512, 65
PARAMS = [(1000, 4), (0, 64), (65535, 0), (65535, 64)]
D_MAX = 300 * (65535 + 64 * 255)


def _records(d, y):
    """The records of 20 x 15 planes [n, 15, 20] -> [n, 300] uint32."""
    d = d.reshape(d.shape[0], 300).astype(np.int64)
    y = y.reshape(y.shape[0], 300).astype(np.int64)
    ok = d > 0
    return (np.where(ok, d, 0) | (y << 16) | (ok.astype(np.int64) << 31)).astype(np.uint32)


def _made_up_planes(n, seed):
    """n planes of 20 x 15: per cell 30 % depth 0, 10 % negative depth, the
    rest valid; the valid depths sit around a per-cell base (differences below
    1000), a fifth of them anywhere in 1 .. 32767 (far above)."""
    rng = np.random.default_rng(seed)
    base = np.random.default_rng(5).integers(2000, 30000, 300)   # the same for every seed
    d = base[None, :] + rng.integers(-700, 701, (n, 300))
    far = rng.random((n, 300)) < 0.2
    d[far] = rng.integers(1, 32768, (n, 300))[far]
    u = rng.random((n, 300))
    d[u < 0.4] = 0
    d[u < 0.1] = rng.integers(-32768, 0, (n, 300))[u < 0.1]
    y = rng.integers(0, 256, (n, 300))
    return d.astype(np.int16).reshape(n, 15, 20), y.astype(np.uint8).reshape(n, 15, 20)


def _made_up():
    """512 stored planes and 65 query planes with, by construction: cells valid
    in both, in one and in neither; |dd| below, at and far above 1000; depths 1
    and 32767; intensities 0 and 255; negative depths; keyframes 6 and 7 alike;
    keyframe 1 all zero; query 1 valid everywhere at intensity 255 (against
    keyframe 1: the largest D there is); query 2 all zero.  Keyframes 0 and 1
    and query 0 carry the edge values, so every n and nq meets some."""
    kd, ky = _made_up_planes(N_STORE, 11)
    qd, qy = _made_up_planes(N_QUERY, 12)
    for d, y in ((kd, ky), (qd, qy)):
        d, y = d.reshape(-1, 300), y.reshape(-1, 300)    # views
        d[0, :8] = [5000, 5000, 5000, 1, 32767, 1, 32767, -32768]
        y[0, :8] = [0, 255, 0, 255, 0, 255, 7, 255]
    k, q = kd.reshape(-1, 300), qd.reshape(-1, 300)
    k[0, :3] = [6000, 5999, 32767]        # against query 0: |dd| = 1000 = cap, 999, 27767
    k[0, 3:5] = [32767, 1]                # 1 against 32767 both ways
    k[1], ky.reshape(-1, 300)[1] = 0, 0
    k[7], ky.reshape(-1, 300)[7] = k[6], ky.reshape(-1, 300)[6]
    q[1], qy.reshape(-1, 300)[1] = 1234, 255
    q[2], qy.reshape(-1, 300)[2] = 0, 0
    sig_k, sig_q = _records(kd, ky), _records(qd, qy)
    # the records are the definition's, on the frames that carry the edges and a few more
    for a in (0, 1, 6, 7, 100, 511):
        assert np.array_equal(sig_k[a], loop_truth.signature(kd[a], ky[a]))
    for a in (0, 1, 2, 64):
        assert np.array_equal(sig_q[a], loop_truth.signature(qd[a], qy[a]))
    assert np.array_equal(sig_k[6], sig_k[7]) and not sig_k[1].any() and (kd < 0).any() and (qd < 0).any()
    dk, yk, vk = loop_truth.fields(sig_k)
    dq, yq, vq = loop_truth.fields(sig_q)
    for d, y, v in ((dk, yk, vk), (dq, yq, vq)):
        assert {1, 32767} <= set(d[v].tolist()) and {0, 255} <= set(y.ravel().tolist())
    both = vq[:, None, :] & vk[None, :, :]
    dd = np.abs(dq[:, None, :] - dk[None, :, :])[both]
    assert (dd == 1000).any() and (dd == 999).any() and (dd < 1000).mean() > 0.3 and (dd > 10000).mean() > 0.05
    assert (dd == 0).any() and dd.max() == 32766
    return dict(kd=kd, ky=ky, qd=qd, qy=qy, sig_k=sig_k, sig_q=sig_q, vk=vk, vq=vq, want={})


@pytest.fixture(scope="module")
def made_up():
    return _made_up()


def _want(m, cap, ly):
    """loop_truth.distance of every query against every stored record, once."""
    if (cap, ly) not in m["want"]:
        m["want"][cap, ly] = np.array([[loop_truth.distance(a, b, cap, ly) for b in m["sig_k"]]
                                       for a in m["sig_q"]], np.int64)
    return m["want"][cap, ly]


def _dev_planes(d, y):
    """Device copies, complete before the closer's own (non-blocking) stream reads them."""
    td, ty = torch.from_numpy(d).cuda(), torch.from_numpy(y).cuda()
    torch.cuda.synchronize()
    return td, ty


def _add(lc, td, ty, k):
    return lc.add_keyframe_device(td.data_ptr() + 2 * 300 * k, ty.data_ptr() + 300 * k, np.eye(4), tag=k)


@pytest.mark.parametrize("cap,ly", PARAMS, ids=lambda v: str(v))
def test_distance_on_made_up_records(made_up, cap, ly):
    """Every (n, nq) of the lists below inside one store of 512: D is [nq, n],
    so a row stride taken from the capacity, 512, shows at every n below it."""
    m = made_up
    want = _want(m, cap, ly)
    assert want.max() < 2 ** 32
    if (cap, ly) == (65535, 64):
        assert want[1, 1] == D_MAX == want.max()      # all 300 cells: one valid, 255 against 0
    td, ty = _dev_planes(m["kd"], m["ky"])
    with youth_loop.LoopCloser(20, 15, N_STORE, cap=cap, ly=ly) as lc:
        for n in (1, 2, 63, 64, 65, 512):
            while lc.keyframes() < n:
                k = lc.keyframes()
                assert _add(lc, td, ty, k) == k
            for nq in (1, 3, 65):
                both = (m["vq"][:nq, None, :] & m["vk"][None, :n, :]).mean()
                one = (m["vq"][:nq, None, :] ^ m["vk"][None, :n, :]).mean()
                assert min(both, one, 1.0 - both - one) >= 0.1, (n, nq, both, one)
                D = lc.distances(m["sig_q"][:nq])
                assert D.shape == (nq, n) and D.dtype == np.uint32
                bad = np.argwhere(D != want[:nq, :n])
                assert bad.size == 0, (n, nq, bad[:5], D[tuple(bad[0])], want[tuple(bad[0])])
        assert lc.keyframe(511)[1] == 511
    both = (m["vq"][:, None, :] & m["vk"][None, :, :]).mean()
    one = (m["vq"][:, None, :] ^ m["vk"][None, :, :]).mean()
    print(f"cells valid in both {both:.3f}, in one {one:.3f}, in neither {1 - both - one:.3f}")
    assert min(both, one, 1.0 - both - one) >= 0.1


def test_distance_after_clear(made_up):
    m = made_up
    td, ty = _dev_planes(m["kd"], m["ky"])
    with youth_loop.LoopCloser(20, 15, 8) as lc:
        for k in (0, 1, 2):
            _add(lc, td, ty, k)
        assert np.array_equal(lc.distances(m["sig_q"][:3]), _want(m, 1000, 4)[:3, :3])
        lc.clear()
        assert lc.keyframes() == 0 and lc.distances(m["sig_q"][:3]).shape == (3, 0)
        assert lc.edges().shape == (0,) and lc.last_verified().shape == (0,)
        # slot 0 again, and its new record is the one compared
        assert _add(lc, td, ty, 100) == 0 and lc.keyframes() == 1
        D = lc.distances(m["sig_q"][:3])
        assert D.shape == (3, 1) and np.array_equal(D[:, 0], _want(m, 1000, 4)[:3, 100])
        assert not np.array_equal(D[:, 0], _want(m, 1000, 4)[:3, 0])
        assert lc.keyframe(0)[1] == 100


def test_candidates_at_the_limit_and_in_ties():
    """cap 1000, ly 4, max_cell_dist 10: D = 3000 is a candidate, 3001 is not."""
    q = np.full(300, 5000, np.int64), np.full(300, 100, np.int64)

    def frame(depth=(), gray=()):
        d, y = q[0].copy(), q[1].copy()
        for c, v in depth:
            d[c] = v
        for c, v in gray:
            y[c] = v
        return d, y

    at = frame(depth=[(0, 6000), (1, 7000), (2, 4000)])               # 3 x 1000 (one capped)
    above = frame(depth=[(0, 6000), (1, 6000), (2, 6000), (3, 5001)])  # 3001
    tie = frame(depth=[(0, 6000), (299, 0)])                          # 1000 + cap for the lost cell
    near = frame(gray=[(7, 101)])                                     # 4
    far = frame(depth=[(c, -1) for c in range(300)])                  # 300 000
    frames = [at, tie, above, tie, tie, near, tie, far, tie, q, q, q]
    d = np.array([f[0] for f in frames]).astype(np.int16).reshape(-1, 15, 20)
    y = np.array([f[1] for f in frames]).astype(np.uint8).reshape(-1, 15, 20)
    sig = _records(d, y)
    want_D = [3000, 2000, 3001, 2000, 2000, 4, 2000, 300000, 2000, 0, 0, 0]
    assert [loop_truth.distance(sig[11], s) for s in sig] == want_D
    td, ty = _dev_planes(d, y)
    with youth_loop.LoopCloser(20, 15, 16, min_gap=2, max_candidates=16, max_cell_dist=10) as lc:
        for k in range(12):
            _add(lc, td, ty, k)
        D = lc.distances(sig[11:12])[0]
        assert D.tolist() == want_D
        idx, dist = lc.candidates(11)
        want = loop_truth.candidates(D, 11, 2, 10, 16)
        assert want == [9, 5, 1, 3, 4, 6, 8, 0]       # 10: too near; 2, 7: over the limit
        assert idx.tolist() == want and dist.tolist() == [0, 4, 2000, 2000, 2000, 2000, 2000, 3000]
        for k in (0, 1, 3, 7):
            idx, dist = lc.candidates(11, k)
            assert idx.tolist() == want[:k] and dist.tolist() == [want_D[c] for c in want[:k]]
        # min_gap larger than the keyframe's index
        assert lc.candidates(1)[0].shape == (0,) and lc.candidates(0)[0].shape == (0,)
        assert lc.candidates(2)[0].tolist() == loop_truth.candidates(lc.distances(sig[2:3])[0], 2, 2, 10, 16)
    # max_candidates below the number that qualify cuts the same list
    with youth_loop.LoopCloser(20, 15, 16, min_gap=2, max_candidates=4, max_cell_dist=10) as lc:
        for k in range(12):
            _add(lc, td, ty, k)
        assert lc.candidates(11)[0].tolist() == want[:4] and lc.candidates(11, 2)[0].tolist() == want[:2]


# -------------------------------------------------------- the C5 keyframe graph --
@pytest.fixture(scope="module")
def c5():
    """The 17 keyframes (C5 frames 0, 40, ..., 600, 630 at 160 x 120) stored with
    their ground-truth poses, every keyframe from 2 on closed, min_gap 2."""
    K = youth_icp.Intrinsics(*K160)
    fr, X, rgb = [], [], []
    for f in loop_truth.KF_FRAMES:
        a, T, c = youth_synth.sequence_rgb(f, 1, 160, 120, K=K)
        fr.append(a[0]), X.append(T[0]), rgb.append(c[0])
    fr, X, rgb = np.array(fr), np.array(X), np.array(rgb)
    gray = youth_synth.luma(rgb)
    sigs = np.array([loop_truth.signature(fr[k], gray[k]) for k in range(17)])
    with youth_loop.LoopCloser(160, 120, 32, K=K, min_gap=2) as lc:
        for k in range(17):
            assert lc.add_keyframe(fr[k], rgb[k], X[k], tag=loop_truth.KF_FRAMES[k]) == k
        D = lc.distances(sigs)
        cands = [lc.candidates(q) for q in range(17)]
        added, verified = {}, {}
        for q in range(2, 17):
            added[q] = lc.close(q)
            verified[q] = lc.last_verified()
        edges = lc.edges()
        T5, tag5 = lc.keyframe(5)
    return dict(fr=fr, X=X, rgb=rgb, gray=gray, sigs=sigs, D=D, cands=cands, added=added,
                verified=verified, edges=edges, T5=T5, tag5=tag5, K=K)


def test_distances_are_bit_exact(c5):
    want = np.array([[loop_truth.distance(c5["sigs"][q], c5["sigs"][k]) for k in range(17)]
                     for q in range(17)], np.uint32)
    assert c5["D"].shape == (17, 17) and np.array_equal(c5["D"], want)
    assert (np.diag(want) == 0).all() and want[16, 0] == want[0, 16] > 0
    print("D(16, k):", want[16].tolist())
    assert c5["tag5"] == 200 and np.array_equal(c5["T5"], c5["X"][5])


def test_candidates_follow_the_definition(c5):
    P = youth_loop.default_params()
    for q in range(17):
        idx, dist = c5["cands"][q]
        want = loop_truth.candidates(c5["D"][q], q, 2, P.max_cell_dist, P.max_candidates)
        assert idx.tolist() == want, q
        assert dist.tolist() == [int(c5["D"][q][k]) for k in want]
    # the revisit is frame 630's best candidate
    assert c5["cands"][16][0][0] == 0


def test_candidate_ties_go_to_the_lower_index(c5):
    fr, rgb, X = c5["fr"], c5["rgb"], c5["X"]
    with youth_loop.LoopCloser(160, 120, 8, K=c5["K"], min_gap=1, max_candidates=3) as lc:
        for k in (1, 0, 0, 2, 16):   # frame 0 stored twice, at indices 1 and 2
            lc.add_keyframe(fr[k], rgb[k], X[k])
        idx, dist = lc.candidates(4)
        D = lc.distances(c5["sigs"][16:17])[0]
    assert D[1] == D[2] == c5["D"][16, 0]
    want = loop_truth.candidates(D, 4, 1, 400, 3)
    assert idx.tolist() == want and idx.tolist()[:2] == [1, 2] and dist[0] == dist[1]


def test_close_finds_the_revisit_and_nothing_else(c5):
    edges, X = c5["edges"], c5["X"]
    for q, v in c5["verified"].items():
        for e in v:
            print(f"({e['i']:2d}, {e['j']:2d}) w {e['w']:.0f} overlap {e['overlap']:.3f} grey rms "
                  f"{e['gray_rms']:.2f} fb {e['fb_rot_deg']:.4f} deg / {e['fb_trans_m'] * 1e3:.3f} mm")
    assert c5["added"][16] >= 1
    assert [(int(e["i"]), int(e["j"])) for e in edges] == [(0, 16)]
    assert sum(c5["added"].values()) == 1
    e = edges[0]
    P = youth_loop.default_params()
    assert e["w"] == 1.0 and e["overlap"] >= P.min_overlap and e["gray_rms"] <= P.max_gray_rms
    assert e["fb_rot_deg"] <= P.fb_rot_deg and e["fb_trans_m"] <= P.fb_trans_m
    # the edge is the RGB-D alignment of frame 630 onto frame 0 ...
    T64, _, st, _ = rgbd_truth.align(c5["fr"][16], c5["gray"][16], c5["fr"][0], c5["gray"][0], K=c5["K"])
    print("max |Z - numpy align|:", np.abs(e["Z"] - T64).max())
    assert st == 0 and np.abs(e["Z"] - T64).max() <= 1e-5
    # ... and the true relative pose
    deg, mm = loop_truth.pose_error(e["Z"], np.linalg.inv(X[0]) @ X[16])
    print(f"edge (0, 16) against the truth: {deg:.4f} deg / {mm:.3f} mm")
    assert deg <= 0.05 and mm <= 1.0


def test_the_edge_pulls_biased_odometry_shut(c5):
    X, e = c5["X"], c5["edges"][0]
    odo = loop_truth.odometry_edges(X, loop_truth.BIAS)
    Xb = loop_truth.compose(odo, X[0])
    edges = youth_loop.make_edges(odo + [(int(e["i"]), int(e["j"]), e["Z"], 1.0)])
    Xo, c0, c1 = youth_loop.optimize_pose_graph(Xb, edges)
    before = loop_truth.pose_error(Xb[16], X[16])
    after = loop_truth.pose_error(Xo[16], X[16])
    print("node 16: %.3f deg / %.2f mm -> %.3f deg / %.2f mm" % (*before, *after))
    assert c1 < c0 and after[0] < before[0] / 4 and after[1] < before[1] / 4
