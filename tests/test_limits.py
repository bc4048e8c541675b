"""The CPU half of test_gpu_limits.py: tests/limit_frames.py's constructions
against the truth modules at small sizes, and the counters that show each GPU
case reaches what it is for.  No GPU."""
import numpy as np
import pytest

import filter_truth as ft
import limit_frames as lf
import loop_truth
import map_truth
import rectify_truth
import render_truth
import youth_icp


# ------------------------------------------------------------ periodic frames --

def _filter(rows):
    return ft.filter_truth(rows, 8, 96)


@pytest.mark.parametrize("W,H,B,phase", [(97, 53, 10, 0), (97, 53, 10, 7), (24, 16, 4, 1), (33, 200, 100, 5)])
def test_periodic_truth_is_the_whole_frames_truth_under_the_filter(W, H, B, phase):
    """The lemma behind the 2^26-pixel filter cases: interior repeats from the
    block with its wrapped halo, the top and bottom rows from two strips."""
    block = lf.depth_block(B, W, W + H)
    frame = lf.periodic_frame(block, H, phase)
    assert np.array_equal(frame[B:2 * B], frame[:B]) or H < 2 * B
    parts = lf.periodic_truth(_filter, block, H, 2, phase)
    want = _filter(frame)
    assert np.array_equal(lf.expand(*parts, H, phase), want)
    assert int((want != frame).sum()) > W * H // 8            # the filter did filter
    # a reach one row short is not enough: the lemma is not vacuous
    short = lf.periodic_truth(_filter, block, H, 1, phase)
    assert not np.array_equal(lf.expand(*short, H, phase), want)
    # the interior does not depend on the phase
    again = lf.periodic_truth(_filter, block, H, 2, phase + 3, interior=parts[0])
    assert np.array_equal(lf.expand(*again, H, phase + 3), _filter(lf.periodic_frame(block, H, phase + 3)))


@pytest.mark.parametrize("W,H,B", [(37, 53, 10), (8, 31, 3)])
def test_periodic_truth_under_the_photometric_prep(W, H, B):
    block = lf.rgb_block(B, W, W)
    whole = lf.photo_words(lf.periodic_frame(block, H, 3))
    parts = lf.periodic_truth(lf.photo_words, block, H, 1, 3)
    assert np.array_equal(lf.expand(*parts, H, 3), whole)
    assert int((whole < 0).sum()) == (W - 2) * (H - 2)         # the valid bit off on the border only


# ------------------------------------------------- 65535 tiny frames as one --

def test_stacked_frames_filter_as_single_frames():
    frames = lf.counter_depth(50, 3, 3)
    got = lf.unstack(_filter(lf.stack_with_gaps(frames, 2)), 50, 3, 2)
    assert np.array_equal(got, _filter(frames))
    assert int((got != frames).sum()) > 50
    # one row of zeros between the frames is too little
    one = lf.unstack(_filter(lf.stack_with_gaps(frames, 1)), 50, 3, 1)
    assert not np.array_equal(one, got)
    all_frames = lf.counter_depth(lf.MAX_FRAMES, 3, 3)
    assert len(np.unique(all_frames.reshape(lf.MAX_FRAMES, -1), axis=0)) > lf.MAX_FRAMES // 2


def test_tiled_map_parts_rectify_as_single_frames():
    W, H, n = 2, 2, 40
    K, Ko = (1.0, 1.25, 0.45, 0.4, 1000.0), (2.0, 2.5, 0.1, 0.2, 1000.0)
    D = (-0.2, 0.02, 0.01, -0.01, 0.0)
    parts = rectify_truth.map_parts(W, H, K, D, Ko)
    assert parts[0].all() and (parts[3] % 32 != 0).all() and (parts[4] % 32 != 0).all()
    d = lf.counter_depth(n, H, W)
    d = np.where(d > 0, 1500 + d % 16, d).astype(np.int16)
    c = (np.arange(n * 12, dtype=np.int64) * 37 % 256).astype(np.uint8).reshape(n, H, W, 3)
    wide = lf.tile_parts(parts, n)
    got_d = lf.from_side_by_side(rectify_truth.rectify_depth(lf.side_by_side(d), wide), n)
    got_c = lf.from_side_by_side(rectify_truth.rectify_color(lf.side_by_side(c), wide), n)
    want_d, want_c = rectify_truth.rectify(d, c, W, H, K, D, Ko)
    assert np.array_equal(got_d, want_d) and np.array_equal(got_c, want_c)
    assert int((want_d != d).sum()) > n
    # a map with uncovered pixels as well
    W, H = 5, 4
    K = (4.0, 4.0, 2.2, 1.7, 1000.0)
    parts = rectify_truth.map_parts(W, H, K, (0.3, 0.0, 0.02, 0.0, 0.0))
    assert 0 < parts[0].sum() < W * H
    d = lf.counter_depth(n, H, W)
    wide = lf.tile_parts(parts, n)
    got = lf.from_side_by_side(rectify_truth.rectify_depth(lf.side_by_side(d), wide), n)
    assert np.array_equal(got, rectify_truth.rectify(d, None, W, H, K, (0.3, 0.0, 0.02, 0.0, 0.0))[0])


def test_signature_of_20x15_frames_is_the_pixel():
    n = 60
    d = lf.counter_depth(n, 15, 20)
    d[3] = 0
    d[4, 2, 5] = 32767
    y = (np.arange(n * 300, dtype=np.int64) * 13 % 256).astype(np.uint8).reshape(n, 15, 20)
    want = np.array([loop_truth.signature(d[k], y[k]) for k in range(n)])
    assert np.array_equal(lf.signature_20x15(d, y), want)
    assert (want[3] >> 31 == 0).all() and (want[0] >> 31).any()


def test_identity_map_under_the_exact_camera():
    for W, H in lf.BIG + [(97, 53)]:
        assert lf.identity_map_holds(W, H, (8192.0, 8192.0, float(W // 2), float(H // 2), 1000.0))
    # a focal length that is no power of two rounds: the lemma notices
    assert not lf.identity_map_holds(8192, 8192, (5734.4, 5734.4, 4096.0, 4096.0, 1000.0))
    # and at small size the whole map is the identity: every weight on tap 00
    # but in the last column and row, where the clamp moves it
    cov, ix, iy, a, b = rectify_truth.map_parts(97, 53, (8192.0, 8192.0, 48.0, 26.0, 1000.0),
                                                (0.0,) * 5)
    assert cov.all() and np.array_equal(ix * 32 + a, np.broadcast_to(np.arange(97) * 32, (53, 97)))
    assert np.array_equal(iy * 32 + b, np.broadcast_to(np.arange(53)[:, None] * 32, (53, 97)))


# ------------------------------------------------------------------ counters --

def test_shapes_are_what_the_units_admit():
    for m, mh in ((1, None), (2, None), (3, None), (20, 15)):
        for W, H in lf.shapes(m, mh):
            assert lf.admitted(W, H, m, mh)
    assert not lf.admitted(16385, 1, 1) and not lf.admitted(8192, 8193, 1) and not lf.admitted(2, 16384, 3)
    assert lf.admitted(8191, 8193, 1) and 8191 * 8193 == lf.MAX_PIXELS - 1


def test_smallest_batches_past_32_bits():
    """The table of case B: the last frame's byte offset no longer fits 32
    bits, the frame before it still does."""
    N = lf.MAX_PIXELS
    for what, frame_bytes, n in (("viewer vertices", 24 * N, 4), ("z-buffer", 8 * N, 9),
                                 ("filter depth", 2 * N, 33), ("map depth", 2 * N, 33),
                                 ("map colour", 3 * N, 23), ("rectifier colour", 3 * N, 23)):
        assert lf.smallest_batch_past_32_bits(frame_bytes) == n, what
        assert lf.last_frame_offset(n, frame_bytes) >= 1 << 32 > lf.last_frame_offset(n - 1, frame_bytes)
    for n in (4, 9, 23, 33):
        k = lf.batch_kinds(n)
        assert k[0] == 0 and k[n - 2] == 2 and k[n - 1] == 3 and (k[1:n - 2] == 1).all()


@pytest.mark.parametrize("shape", lf.shapes(1) + [(8191, 8193)], ids=lf.shape_id)
def test_sparse_frames_reach_the_corners_the_last_tile_and_the_long_scan(shape):
    W, H = shape
    N = W * H
    idx = lf.sparse_pixels(W, H, 20_000, 17 + W)
    assert (np.diff(idx) > 0).all() and idx[0] == 0 and idx[-1] == N - 1
    for px in (4, 8):
        cnt = lf.sparse_counters(idx, W, H, 256 * px)
        assert cnt["corners"] and cnt["last_tile_valid"] >= 1
        if N >= lf.MAX_PIXELS - 1:
            assert cnt["R"] == (128 if px == 8 else 256)       # k_cloud_scan's run length
        assert cnt["last_tile_partial"] == (shape == (8191, 8193))
    if shape == (8191, 8193):
        assert N % 4 and N % 8                                  # the scalar-load path
    if N <= 1 << 14:
        d = lf.sparse_depth(W, H, idx, 5)
        c = lf.sparse_rgb(W, H, idx, 5)
        assert np.array_equal(np.flatnonzero(d.reshape(-1) > 0), idx) and (d < 0).any()
        assert not c.reshape(-1, 3)[d.reshape(-1) <= 0].any()


def test_boundary_points_fall_in_their_classes():
    """DESIGN.md §10's key at 2^20 voxels per metre: -1.0 in cell -2^20,
    nextafter(1, 0) in cell 2^20 - 1 with q = 240, 1.0 and nextafter(-1, -2)
    out of range; the 1 x 1 frames reproduce the points exactly."""
    f = np.float32
    ok, cell, q = map_truth.keys_of(np.array([[-1.0, np.nextafter(f(1), f(0)), 0.0]], f), lf.BOUNDARY_VPM)
    assert ok.all() and cell.tolist() == [[lf.CELL_MIN, lf.CELL_MAX, 0]] and q.tolist() == [[0, 240, 0]]
    for bad in (f(1.0), np.nextafter(f(-1), f(-2))):
        assert not map_truth.keys_of(np.array([[bad, 0.0, 0.0]], f), lf.BOUNDARY_VPM)[0].any()
    P, cls = lf.boundary_points()
    assert dict(zip(*np.unique(cls, return_counts=True))) == {"corner": 8, "near": 3, "out": 6, "ordinary": 8}
    ok, cell, q = map_truth.keys_of(P, lf.BOUNDARY_VPM)
    assert ok[cls != "out"].all() and not ok[cls == "out"].any()
    assert len({tuple(c) for c in cell[:8]}) == 8 and set(np.unique(cell[:8])) == {lf.CELL_MIN, lf.CELL_MAX}
    near = cell[8:11]
    assert (near == lf.CELL_MIN).sum() == 3 and (near == lf.CELL_MAX).sum() == 3
    # exactly one axis puts an `out` point out of range
    s = P[cls == "out"] * f(lf.BOUNDARY_VPM)
    fl = np.floor(s)
    assert (((fl < -1048576) | (fl >= 1048576)).sum(axis=1) == 1).all()
    depth, rgb, T = lf.point_frames(P)
    got = np.concatenate([map_truth.frame_points(depth[k], rgb[k], None, T[k].reshape(3, 4))[0]
                          for k in range(P.shape[0])])
    assert np.array_equal(got.view(np.uint32), P.view(np.uint32))
    rec, oor = map_truth.restate(P, rgb.reshape(-1, 3), lf.BOUNDARY_VPM)
    assert oor == 6 and rec.shape[0] == 17 and int(rec["count"].sum()) == 19 and rec["count"].max() == 2
    # four corner voxels in front of each of the two views
    K = youth_icp.Intrinsics(16.0, 16.0, 32.0, 32.0, 1000.0)
    for Tw in (np.eye(4), np.diag([-1.0, 1.0, -1.0, 1.0])):
        wd, _ = render_truth.render(rec, lf.BOUNDARY_VPM, render_truth.view_from_pose(Tw), K, 64, 64)
        assert all(wd[y, x] > 0 for y in (16, 48) for x in (16, 48))


def test_smallest_table_frame_is_64_voxels():
    d, c, K = lf.distinct_voxel_frame(64)
    rec, oor = map_truth.restate(*map_truth.frame_points(d, c, youth_icp.Intrinsics(*K)), 1.0)
    assert oor == 0 and rec.shape[0] == 64 and (rec["count"] == 1).all()


def test_queue_cluster_keeps_every_voxel_with_a_whole_footprint():
    """Whatever 1024 of the cluster's voxels the table ends up holding, each
    survives the view's culls with a 16 x 16 footprint inside the frame."""
    depth, rgb = lf.queue_frame()
    rec, oor = map_truth.restate(*map_truth.frame_points(depth, rgb, youth_icp.Intrinsics(*lf.QUEUE_K_IN)),
                                 lf.QUEUE_VPM)
    assert oor == 0 and rec.shape[0] > 10 * lf.QUEUE_SLOTS
    W, H = lf.QUEUE_VIEW
    why = {}
    u0, v0, s, _ = render_truth.project(rec, lf.QUEUE_VPM, np.eye(4)[:3], youth_icp.Intrinsics(*lf.QUEUE_K_VIEW),
                                        W, H, why=why)
    assert why == {"behind": 0, "d_zero": 0, "d_far": 0, "off_frame": 0}
    n = rec.shape[0]
    assert lf.queue_counters(u0, v0, s, n, W, H) == {"records": n, "survivors": n, "whole_16x16": n}
    # 1024 entries of 256 pixels: the queue's last prefix
    assert (lf.QUEUE_SLOTS - 1) * 256 == 261888
