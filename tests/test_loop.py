"""Loop closing on the CPU: the numpy restatement on hand-made
frames with known answers, the gates on hand-made poses and statistics, the
pose graph (libyouth_icp.so, host code) against an independent numpy
Gauss-Newton, on the band of one loop edge and beyond it, the interpolation,
the exports and the stand-alone sanitizer driver of tests/loop_asan."""
import ctypes
import fcntl
import os
import subprocess

import numpy as np
import pytest

import loop_truth
import youth_icp
import youth_loop
import youth_synth
from conftest import PKG, ROOT

VALID = 1 << 31


# ------------------------------------------------------------------ signature --
def _frame(W=40, H=30, depth=1000, gray=100):
    return np.full((H, W), depth, np.int16), np.full((H, W), gray, np.uint8)


def test_signature_of_2x2_cells():
    d, y = _frame()
    # cell (0, 0): pixels (0..1, 0..1); cell (3, 2): columns 6..7, rows 4..5
    d[0:2, 0:2] = [[10, 20], [30, 41]]        # mean 25.25 -> 25
    y[0:2, 0:2] = [[1, 2], [3, 4]]            # (10 + 2) // 4 = 3
    d[4:6, 6:8] = [[10, 20], [30, 42]]        # 25.5 -> 26 (round half up)
    y[4:6, 6:8] = [[255, 255], [255, 254]]    # (1019 + 2) // 4 = 255
    s = loop_truth.signature(d, y)
    assert s.shape == (300,) and s.dtype == np.uint32
    assert s[0] == (25 | (3 << 16) | VALID)
    assert s[2 * 20 + 3] == (26 | (255 << 16) | VALID)
    assert s[1] == (1000 | (100 << 16) | VALID)
    assert s[299] == (1000 | (100 << 16) | VALID)


def test_signature_validity_threshold_and_negative_depths():
    d, y = _frame()
    d[0:2, 0:2] = [[700, 0], [0, 0]]          # 4 cnt = n exactly: valid, dm = 700
    d[0:2, 2:4] = 0                           # wholly invalid
    d[0:2, 4:6] = [[-5, -32768], [-1, 0]]     # negative depths are invalid
    d[0:2, 6:8] = [[-5, 900], [-1, 0]]        # ... and do not enter the sum
    s = loop_truth.signature(d, y)
    assert s[0] == (700 | (100 << 16) | VALID)
    assert s[1] == (100 << 16) and s[2] == (100 << 16)
    assert s[3] == (900 | (100 << 16) | VALID)
    # one pixel below the threshold: 80 x 60 has 4 x 4 cells, 3 of 16 valid
    d, y = _frame(80, 60)
    d[0:4, 0:4] = 0
    d[0, 0:3] = 500
    assert loop_truth.signature(d, y)[0] == (100 << 16)
    d[0, 3] = 500                             # 4 of 16: valid
    assert loop_truth.signature(d, y)[0] == (500 | (100 << 16) | VALID)


def test_signature_ragged_cells_cover_every_pixel_once():
    W, H = 23, 17
    rng = np.random.default_rng(1)
    d = rng.integers(1, 3000, (H, W)).astype(np.int16)
    y = rng.integers(0, 256, (H, W)).astype(np.uint8)
    s = loop_truth.signature(d, y)
    # a cell of one pixel carries that pixel
    assert s[0] == (int(d[0, 0]) | (int(y[0, 0]) << 16) | VALID)
    widths = [(i + 1) * W // 20 - i * W // 20 for i in range(20)]
    heights = [(j + 1) * H // 15 - j * H // 15 for j in range(15)]
    assert sum(widths) == W and sum(heights) == H and min(widths) == 1 and max(widths) == 2


def test_distance_covers_the_three_validity_cases():
    a = np.zeros(300, np.uint32)
    b = np.zeros(300, np.uint32)
    a[0], b[0] = 1000 | (10 << 16) | VALID, 1300 | (14 << 16) | VALID   # both: 300 + 4 * 4
    a[1], b[1] = 1000 | (10 << 16) | VALID, 4000 | (10 << 16) | VALID   # both, capped: 1000
    a[2], b[2] = 1000 | (200 << 16) | VALID, (190 << 16)                # one: 1000 + 40
    a[3], b[3] = (7 << 16), (9 << 16)                                   # neither: 0 + 8
    assert loop_truth.distance(a, b) == 316 + 1000 + 1040 + 8
    assert loop_truth.distance(b, a) == loop_truth.distance(a, b)
    assert loop_truth.distance(a, a) == 0
    assert loop_truth.distance(a, b, cap=100, ly=1) == (100 + 4) + 100 + (100 + 10) + 2
    # the bound of the header: 300 cells of cap + ly * 255
    full = np.full(300, 65535 | VALID, np.uint32)
    none = np.full(300, 255 << 16, np.uint32)
    assert loop_truth.distance(full, none) == 300 * (1000 + 4 * 255) == 606000


def test_candidate_order_breaks_ties_by_index():
    D = np.array([500, 300, 300, 130000, 100, 50], np.uint32)
    assert loop_truth.candidates(D, 5, 2, 400, 4) == [1, 2, 0]       # 3: over the limit; 4, 5: too near
    assert loop_truth.candidates(D, 5, 1, 400, 2) == [4, 1]


# ---------------------------------------------------------------------- gates --
def _rot_z(deg, t):
    a = np.radians(deg)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = t
    return T


def test_gates_on_hand_made_poses_and_statistics():
    """Known angle and norm of T_fwd T_bwd (the other order has another norm),
    the forward direction with the smaller overlap AND the smaller RMS, so min
    and max pick different directions; a [iters, 4] array means its last row."""
    Tf, Tb = _rot_z(40.0, (0.1, 0.0, 0.0)), _rot_z(-10.0, (0.0, 0.2, 0.05))
    s40, c40, s10, c10 = np.sin(np.radians(40)), np.cos(np.radians(40)), np.sin(np.radians(10)), np.cos(np.radians(10))
    norm = np.sqrt((0.1 - 0.2 * s40) ** 2 + (0.2 * c40) ** 2 + 0.05 ** 2)
    other = np.sqrt((0.1 * c10) ** 2 + (0.2 - 0.1 * s10) ** 2 + 0.05 ** 2)
    assert abs(norm - other) > 0.02
    fwd = [7.0, 1000.0, 0.0009, 900.0]      # 1000 of 4000 pixels; 2550 sqrt(1e-6) = 2.55
    bwd = [3.0, 2000.0, 0.0064, 1600.0]     # 2000 of 4000 pixels; 2550 sqrt(4e-6) = 5.10
    ov, rms, deg, m = loop_truth.gates(Tf, fwd, Tb, bwd, 4000, 0.1)
    assert abs(ov - 0.25) <= 1e-15 and abs(rms - 5.1) <= 1e-12
    assert abs(deg - 30.0) <= 1e-12 and abs(m - norm) <= 1e-15
    # the directions swapped: overlap and RMS stay, the product's translation does not
    ov2, rms2, deg2, m2 = loop_truth.gates(Tb, bwd, Tf, fwd, 4000, 0.1)
    assert (ov2, rms2) == (ov, rms) and abs(deg2 - 30.0) <= 1e-12 and abs(m2 - other) <= 1e-15
    # a last row that is not (0, 0, 0, 1) is replaced; [3, 4] poses do as well
    bad = Tf.copy()
    bad[3] = (9.0, -9.0, 9.0, 9.0)
    assert loop_truth.gates(bad, fwd, Tb[:3], bwd, 4000, 0.1) == (ov, rms, deg, m)
    # the last iteration's row of a table, not the first
    table = np.array([[1.0, 4000.0, 1.0, 4000.0], [2.0, 3000.0, 0.5, 10.0], fwd])
    assert loop_truth.gates(Tf, table, Tb, bwd, 4000, 0.1) == (ov, rms, deg, m)
    # no photometric pixel one way: the RMS is infinite, the rest stands
    none = [7.0, 1000.0, 0.0, 0.0]
    ov3, rms3, deg3, m3 = loop_truth.gates(Tf, none, Tb, bwd, 4000, 0.1)
    assert rms3 == np.inf and (ov3, deg3, m3) == (ov, deg, m)
    assert loop_truth.gates(Tf, fwd, Tb, none, 4000, 0.1)[1] == np.inf
    # lambda scales the RMS back to grey levels; identical poses inverse to each other: 0, 0
    assert abs(loop_truth.gates(Tf, fwd, Tb, bwd, 4000, 0.2)[1] - 2.55) <= 1e-12
    _, _, deg0, m0 = loop_truth.gates(Tf, fwd, np.linalg.inv(Tf), bwd, 4000, 0.1)
    assert deg0 <= 1e-12 and m0 <= 1e-15


# ----------------------------------------------------------------- pose graph --
@pytest.fixture(scope="module")
def graph():
    """The 17 ground-truth poses of C5 frames 0, 40, ..., 600, 630."""
    X = np.array([youth_synth.sequence(f, 1, 32, 24)[1][0] for f in loop_truth.KF_FRAMES])
    assert X.shape == (17, 4, 4)
    loop = (0, 16, np.linalg.inv(X[0]) @ X[16], 1.0)
    return X, loop


def test_posegraph_leaves_an_exact_graph_alone(graph):
    X, loop = graph
    edges = loop_truth.odometry_edges(X) + [loop]
    Xo, c0, c1 = youth_loop.optimize_pose_graph(X, youth_loop.make_edges(edges))
    print("exact graph: cost", c0, "->", c1, " max |dX|", np.abs(Xo - X).max())
    assert np.abs(Xo - X).max() <= 1e-9 and c0 <= 1e-20 and c1 <= 1e-20


def test_posegraph_matches_numpy_and_pulls_the_loop_shut(graph):
    X, loop = graph
    odo = loop_truth.odometry_edges(X, loop_truth.BIAS)
    Xb = loop_truth.compose(odo, X[0])
    edges = odo + [loop]
    Xo, c0, c1 = youth_loop.optimize_pose_graph(Xb, youth_loop.make_edges(edges))
    want = loop_truth.optimize(Xb, edges)
    print("max |C - numpy|:", np.abs(Xo - want).max())
    assert np.abs(Xo - want).max() <= 1e-8
    assert abs(c0 - loop_truth.cost(Xb, edges)) <= 1e-12 and abs(c1 - loop_truth.cost(Xo, edges)) <= 1e-12
    print("cost", c0, "->", c1)
    assert c1 < c0
    before = np.array([loop_truth.pose_error(Xb[k], X[k]) for k in range(17)])
    after = np.array([loop_truth.pose_error(Xo[k], X[k]) for k in range(17)])
    print("node 16: %.3f deg / %.2f mm -> %.3f deg / %.2f mm" % (*before[16], *after[16]))
    assert after[16][0] < before[16][0] / 4 and after[16][1] < before[16][1] / 4
    assert after[:, 0].max() <= before[:, 0].max() and after[:, 1].max() <= before[:, 1].max()
    # node 0 is the gauge
    assert np.array_equal(Xo[0], Xb[0])


# Beyond the band.  With the one loop edge (0, 16) H stays block-tridiagonal:
# node 0 has no columns.  These graphs have loop edges between free nodes, so H
# gets off-diagonal blocks far from the diagonal and cholesky_solve's envelope
# long rows; edges given with i > j; weights other than 1; w_rot != w_trans.
def _beyond_the_band(n, seed):
    """A random chain of n nodes (steps of about 0.15 rad and 0.3 m, node 0 not
    the identity), its biased odometry with weights from {0.5, 1, 2}, and the
    loop edges: (2, n - 3) and (2, n // 2 + 1) share node 2, (n - 2, 3) is given
    with i > j, (0, n - 4) touches the gauge, (n - 3, 1) has a pure rotation for
    Z (nodes 1 and n - 3 share a camera centre), and (4, 7) has weight 0 and a
    random Z.  The loop edges' Z carry a little noise, so they pull against each
    other.  -> (X_true, X_start, edges, index of the zero-weight edge, index of
    the pure-rotation edge)."""
    rng = np.random.default_rng(seed)
    X = [loop_truth.se3_exp(rng.normal(0, 0.3, 6))]
    for _ in range(1, n):
        xi = np.concatenate([rng.normal(0, 0.15 / np.sqrt(3), 3), rng.normal(0, 0.3 / np.sqrt(3), 3)])
        X.append(X[-1] @ loop_truth.se3_exp(xi))
    X = np.array(X)
    X[n - 3][:3, 3] = X[1][:3, 3]
    odo = [(i, j, Z, float(rng.choice([0.5, 1.0, 2.0]))) for i, j, Z, _ in
           loop_truth.odometry_edges(X, loop_truth.BIAS)]
    Xb = loop_truth.compose(odo, X[0])
    loops = []
    for i, j in ((2, n - 3), (2, n // 2 + 1), (n - 2, 3), (0, n - 4)):
        Z = np.linalg.inv(X[i]) @ X[j] @ loop_truth.se3_exp(rng.normal(0, 0.003, 6))
        loops.append((i, j, Z, float(rng.choice([0.5, 1.0, 2.0]))))
    Z = np.linalg.inv(X[n - 3]) @ X[1]
    assert np.abs(Z[:3, 3]).max() <= 1e-15
    Z[:3, 3] = 0.0
    Z[:3, :3] = Z[:3, :3] @ loop_truth.exp_so3(rng.normal(0, 0.003, 3))
    loops.append((n - 3, 1, Z, 2.0))
    loops.append((4, 7, loop_truth.se3_exp(rng.normal(0, 1.0, 6)), 0.0))
    edges = odo + loops
    assert {w for *_, w in edges} >= {0.0, 0.5, 1.0, 2.0}
    return X, Xb, edges, len(edges) - 1, len(edges) - 2


@pytest.mark.parametrize("w_rot,w_trans", [(1.0, 1.0), (3.0, 0.5)], ids=lambda v: str(v))
@pytest.mark.parametrize("n", [9, 12, 20])
def test_posegraph_beyond_the_band_matches_numpy(n, w_rot, w_trans):
    """Worst observed over the six cases: poses 4.5e-12, costs 1.2e-15
    (bars: 1e-8 and 1e-12, those of the band test above)."""
    X, Xb, edges, zero, _ = _beyond_the_band(n, 100 + n)
    Xo, c0, c1 = youth_loop.optimize_pose_graph(Xb, youth_loop.make_edges(edges), w_rot, w_trans)
    want = loop_truth.optimize(Xb, edges, w_rot, w_trans)
    d0 = abs(c0 - loop_truth.cost(Xb, edges, w_rot, w_trans))
    d1 = abs(c1 - loop_truth.cost(Xo, edges, w_rot, w_trans))
    print(f"n {n}: max |C - numpy| {np.abs(Xo - want).max():.2e}, costs {d0:.1e} {d1:.1e}; {c0:.4g} -> {c1:.4g}")
    assert np.abs(Xo - want).max() <= 1e-8
    assert d0 <= 1e-12 and d1 <= 1e-12 and c1 < c0
    # the loop edges moved the nodes: this is no fixed point of the start
    assert np.abs(Xo - Xb).max() > 1e-3
    # node 0 is the gauge
    assert np.array_equal(Xo[0], Xb[0])
    # an edge of weight 0 counts for nothing, whatever its Z
    rest = edges[:zero] + edges[zero + 1:]
    Xr, r0, r1 = youth_loop.optimize_pose_graph(Xb, youth_loop.make_edges(rest), w_rot, w_trans)
    assert np.abs(Xr - Xo).max() <= 1e-12 and abs(r0 - c0) <= 1e-12 and abs(r1 - c1) <= 1e-12


@pytest.mark.parametrize("n", [9, 12, 20])
def test_posegraph_reversed_edges(n):
    """(i, j, Z, w) and (j, i, Z^-1, w) state the same measurement.  The reversed
    edge's residual is E' = Z E^-1 Z^-1: its rotation vector is -R_Z e_w, of the
    same length, and its translation is (I - R_Z R_E^T R_Z^T) t_Z - R_Z R_E^T t_E,
    of the same length where t_Z = 0 or R_E = I.  So the cost, and with it the
    optimum, is the same function for the pure-rotation edge (n - 3, 1) whatever
    the weights, which is what is asserted (1e-8, the bar between two solvers of
    one problem); for an edge with a lever arm t_Z and a rotation residual left
    at the optimum the two costs differ by the order of |e_w| |t_Z|, so the
    optimum moves (observed: by 6e-4 to 6e-3 with all six loop edges reversed),
    and there the test requires that the C solver and the numpy one still agree
    on the reversed graph.  Worst observed: 1.3e-15 for the pure-rotation edge,
    5.2e-12 against numpy with every loop edge reversed."""
    X, Xb, edges, _, pure = _beyond_the_band(n, 100 + n)
    for w_rot, w_trans in ((1.0, 1.0), (3.0, 0.5)):
        Xo, _, c1 = youth_loop.optimize_pose_graph(Xb, youth_loop.make_edges(edges), w_rot, w_trans)
        i, j, Z, w = edges[pure]
        assert i > j and w == 2.0
        e = loop_truth.residual(Xo[i], Xo[j], Z)
        assert np.linalg.norm(e[:3]) > 1e-4          # it is not at rest at the optimum
        rev = list(edges)
        rev[pure] = (j, i, np.linalg.inv(Z), w)
        Xr, _, r1 = youth_loop.optimize_pose_graph(Xb, youth_loop.make_edges(rev), w_rot, w_trans)
        print(f"n {n} pure-rotation edge reversed: max |dX| {np.abs(Xr - Xo).max():.2e}, cost {abs(r1 - c1):.1e}")
        assert np.abs(Xr - Xo).max() <= 1e-8 and abs(r1 - c1) <= 1e-12
        # every loop edge reversed at once: i > j becomes i < j and the other way round
        m = len(edges) - 6
        rev = edges[:m] + [(j, i, np.linalg.inv(Z), w) for i, j, Z, w in edges[m:]]
        Xr, r0, r1 = youth_loop.optimize_pose_graph(Xb, youth_loop.make_edges(rev), w_rot, w_trans)
        want = loop_truth.optimize(Xb, rev, w_rot, w_trans)
        print(f"n {n} all loop edges reversed: max |C - numpy| {np.abs(Xr - want).max():.2e}, "
              f"against the graph as given {np.abs(Xr - Xo).max():.2e}")
        assert np.abs(Xr - want).max() <= 1e-8
        assert abs(r0 - loop_truth.cost(Xb, rev, w_rot, w_trans)) <= 1e-12
        assert abs(r1 - loop_truth.cost(Xr, rev, w_rot, w_trans)) <= 1e-12


def test_posegraph_at_the_node_limit():
    """512 nodes: exact odometry and one exact loop edge between interior nodes,
    the longest rows the envelope solver can get.  Nothing moves."""
    import time
    rng = np.random.default_rng(512)
    X = [np.eye(4)]
    for _ in range(511):
        xi = np.concatenate([rng.normal(0, 0.15 / np.sqrt(3), 3), rng.normal(0, 0.3 / np.sqrt(3), 3)])
        X.append(X[-1] @ loop_truth.se3_exp(xi))
    X = np.array(X)
    edges = loop_truth.odometry_edges(X) + [(500, 7, np.linalg.inv(X[500]) @ X[7], 2.0)]
    e = youth_loop.make_edges(edges)
    t0 = time.perf_counter()
    Xo, c0, c1 = youth_loop.optimize_pose_graph(X, e)
    dt = time.perf_counter() - t0
    print(f"512 nodes: {dt * 1e3:.0f} ms, max |dX| {np.abs(Xo - X).max():.2e}, cost {c0:.1e} -> {c1:.1e}")
    assert np.abs(Xo - X).max() <= 1e-9 and c0 <= 1e-20 and c1 <= 1e-20
    assert dt < 1.0


def test_posegraph_argument_errors(graph):
    X, loop = graph
    edges = youth_loop.make_edges(loop_truth.odometry_edges(X) + [loop])

    def code(Xin, e):
        with pytest.raises(youth_icp.IcpError) as ei:
            youth_loop.optimize_pose_graph(Xin, e)
        return ei.value.code

    assert code(X[:1], edges[:0]) == youth_icp.YOUTH_EINVAL                  # n < 2
    big = np.tile(np.eye(4), (513, 1, 1))
    assert code(big, edges[:0]) == youth_icp.YOUTH_EINVAL                    # n > 512
    bad = X.copy()
    bad[3, 1, 2] = np.nan
    assert code(bad, edges) == youth_icp.YOUTH_EINVAL
    e = edges.copy()
    e[4]["j"] = 17
    assert code(X, e) == youth_icp.YOUTH_EINVAL
    e = edges.copy()
    e[4]["i"] = -1
    assert code(X, e) == youth_icp.YOUTH_EINVAL
    e = edges.copy()
    e[2]["Z"][0, 3] = np.inf
    assert code(X, e) == youth_icp.YOUTH_EINVAL
    e = edges.copy()
    e[2]["w"] = np.nan
    assert code(X, e) == youth_icp.YOUTH_EINVAL
    # a node no edge reaches: no solution, and X is left alone
    assert code(X, edges[1:16]) == youth_icp.YOUTH_EINVAL


def test_interpolate_rehangs_frames_on_their_keyframe():
    rng = np.random.default_rng(5)
    X = np.array([loop_truth.se3_exp(rng.normal(0, 0.2, 6)) for _ in range(5)])
    kf = [0, 3]
    old = X[kf]
    new = np.array([old[0], loop_truth.se3_exp((0.1, 0.0, -0.2, 0.3, 0.0, 0.1)) @ old[1]])
    got = youth_loop.interpolate(X, kf, old, new)
    for f in range(5):
        k = 0 if f < 3 else 1
        want = new[k] @ np.linalg.inv(old[k]) @ X[f]
        assert np.abs(got[f] - want).max() <= 1e-12, f
    assert np.abs(got[:3] - X[:3]).max() <= 1e-15 and np.abs(got[3] - new[1]).max() <= 1e-12
    with pytest.raises(youth_icp.IcpError):
        youth_loop.interpolate(X, [1, 3], old, new)      # the first keyframe is frame 0
    with pytest.raises(youth_icp.IcpError):
        youth_loop.interpolate(X, [0, 0], old, new)      # ascending


# --------------------------------------------------------------------- exports --
def test_every_declared_symbol_is_exported_and_bound():
    names = youth_icp.declared_functions(youth_loop.HEADER_PATH)
    assert len(names) >= 20 and "youth_loop_close" in names and "youth_posegraph_optimize" in names
    lib = ctypes.CDLL(os.path.join(PKG, "libyouth_icp.so"))
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert sorted(youth_loop._SIGS) == names
    P = youth_loop.default_params()
    assert (P.min_gap, P.max_candidates, P.max_cell_dist, P.cap, P.ly) == (10, 4, 400, 1000, 4)
    assert [round(v, 6) for v in (P.min_overlap, P.max_gray_rms, P.fb_rot_deg, P.fb_trans_m)] == \
        [0.1, 1.5, 0.5, 0.01]
    assert ctypes.sizeof(youth_loop.LoopParams) == 36 and youth_loop.EDGE_DTYPE.itemsize == 176


def test_loop_is_off_without_the_variable():
    assert youth_loop.slam_loop_keyframes() == 0
    assert youth_loop.slam_loop_edges().shape == (0,)
    assert youth_loop.slam_loop_trajectory().shape == (0, 4, 4)


# ------------------------------------------------------------------ sanitizers --
def test_pose_graph_under_asan_and_ubsan():
    """tests/loop_asan: pose_graph.cpp built with -fsanitize=address,undefined
    into a stand-alone program that runs the biased C5 graph and the error
    cases; it exits 0 only when every check holds and no sanitizer fired."""
    d = os.path.join(ROOT, "tests", "loop_asan")
    with open(os.path.join(d, ".build.lock"), "w") as lk:   # one build at a time (parallel workers)
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", d], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(d, "pose_graph_asan")], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "pose graph ok" in r.stdout
