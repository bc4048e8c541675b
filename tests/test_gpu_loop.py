"""Loop closing on the GPU (include/youth_loop.h): the signature
and distance kernels bit for bit against tests/loop_truth.py, the candidate
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
