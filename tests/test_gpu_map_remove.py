"""GPU tests of frame removal from the voxel map (include/youth_map.h,
DESIGN.md §10): k_map_update's removing form, the move, the scan and the
compaction.  A record is integers and every accumulation an unsigned 32-bit
add, so "integrate A, remove B of A" must equal "integrate A without B" bit for
bit: the truth of a removal is map_truth.restate_frames over the frames that
remain, and every comparison is byte equality of the sorted 40-byte records,
as in test_gpu_map.py (whose frame and pose recipes are repeated here).  Every
case asserts stats.dropped == 0, the condition of exactness."""
import functools

import numpy as np
import pytest
import torch

import youth_icp
import youth_map
from map_truth import frame_points, restate, restate_frames

pytestmark = pytest.mark.gpu


def _frame(W, H, seed, holes=0.1, negative=True):
    """The recipe of test_gpu_map.py: random depth with holes and negatives."""
    rng = np.random.default_rng(seed)
    lo = -500 if negative else 0
    depth = rng.integers(lo, 32768, size=(H, W)).astype(np.int16)
    depth[rng.random((H, W)) < holes] = 0
    rgb = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    return depth, rgb


def _pose(rng, big=False):
    """A random camera -> world pose, row-major 3x4 fp32 (test_gpu_map.py)."""
    w = rng.normal(size=3) * (1.0 if big else 0.05)
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / max(th, 1e-12)
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = rng.normal(size=3) * (5.0 if big else 0.1)
    return np.hstack([R, t[:, None]]).astype(np.float32)


def _same(got, want):
    assert got.dtype == want.dtype == youth_map.VOXEL_DTYPE
    assert got.shape == want.shape, (got.shape, want.shape)
    assert got.tobytes() == want.tobytes()


def _points(depth, max_depth=0):
    """Contributing pixels of a frame (none is out of range in these tests)."""
    ok = depth > 0
    return int((ok & (depth <= max_depth)).sum() if max_depth else ok.sum())


def _clean(m, removed=None, vacant=None):
    """Nothing dropped, nothing missing, no underflow, no stale slot."""
    st, rs = m.stats(), m.remove_stats()
    assert st["dropped"] == 0
    assert rs["missing"] == rs["underflow"] == rs["stale"] == 0, rs
    assert rs["live"] + rs["vacant"] == st["occupied"]
    if removed is not None:
        assert rs["removed"] == removed
    if vacant is not None:
        assert rs["vacant"] == vacant
    return st, rs


class _Batch:
    """Frames, their colour and poses on the device, in the given order."""

    def __init__(self, frames, T, order, offset=0):
        n, (H, W) = len(order), frames[0][0].shape
        self.n, self.W, self.H = n, W, H
        self.d = torch.zeros(n * H * W + offset, dtype=torch.int16, device="cuda")
        self.c = torch.zeros(n * H * W * 3 + offset, dtype=torch.uint8, device="cuda")
        self.d[offset:] = torch.from_numpy(np.stack([frames[f][0] for f in order]).reshape(-1)).cuda()
        self.c[offset:] = torch.from_numpy(np.stack([frames[f][1] for f in order]).reshape(-1)).cuda()
        self.T = torch.from_numpy(np.ascontiguousarray(np.stack([T[f] for f in order])).reshape(n, 12)).cuda()
        self.offset = offset
        torch.cuda.synchronize()

    def args(self, first=0, count=None, colour=True):
        """(d_depth, d_rgb, n_frames, W, H, d_T_world) of frames first .. first + count."""
        px = self.W * self.H
        return (self.d.data_ptr() + (self.offset + first * px) * 2,
                self.c.data_ptr() + self.offset + first * px * 3 if colour else 0,
                self.n - first if count is None else count, self.W, self.H,
                self.T.data_ptr() + first * 48)


# ------------------------------------------------------- the four-frame set --
@functools.lru_cache(maxsize=None)
def _four():
    """160 x 120, 4 frames, the random poses of test_many_frames_any_split_any_order."""
    W, H, n, vpm = 160, 120, 4, 100.0
    rng = np.random.default_rng(5)
    frames = [_frame(W, H, 200 + f) for f in range(n)]
    T = np.stack([_pose(rng, big=f % 2 == 1) for f in range(n)])
    K = youth_icp.Intrinsics(525.0, 523.5, 81.25, 59.5, 5000.0)
    truth = {}
    for colour in (True, False):
        for keep in ((0, 1, 2, 3), (0, 2)):
            want, oor = restate_frames([(frames[f][0], frames[f][1] if colour else None, K, T[f])
                                        for f in keep], vpm)
            assert oor == 0
            truth[colour, keep] = want
    return frames, T, K, vpm, truth


def _integrate_four(m, colour=True):
    frames, T, K, vpm, truth = _four()
    b = _Batch(frames, T, range(4))
    a = b.args(colour=colour)
    m.integrate_device(*a[:5], a[5], K)
    return b


# -------------------------------------------------------- 1 subset removal --
@pytest.mark.parametrize("lds,colour", [(True, True), (False, True), (True, False)])
def test_subset_removal_one_call_two_calls_reverse_order(monkeypatch, lds, colour):
    """Integrate frames 0..3, remove {1, 3}: in one call, in two calls and in
    reverse order; each is the restatement of {0, 2}."""
    frames, T, K, vpm, truth = _four()
    if not lds:
        monkeypatch.setenv("YOUTH_MAP_LDS", "0")
    removed = _points(frames[1][0]) + _points(frames[3][0])
    one, rev = _Batch(frames, T, (1, 3)), _Batch(frames, T, (3, 1))
    with youth_map.VoxelMap(vpm) as m:
        for way in ("one call", "two calls", "reverse order"):
            m.clear()
            b = _integrate_four(m, colour)
            _same(m.extract(), truth[colour, (0, 1, 2, 3)])
            if way == "two calls":
                for f in (1, 3):
                    a = b.args(f, 1, colour)
                    m.remove_device(*a[:5], a[5], K)
            else:
                a = (one if way == "one call" else rev).args(colour=colour)
                m.remove_device(*a[:5], a[5], K)
            got = m.extract()
            _same(got, truth[colour, (0, 2)])
            st, rs = _clean(m, removed=removed)
            assert rs["vacant"] > 0 and rs["live"] == got.shape[0]
            assert st["occupied"] == truth[colour, (0, 1, 2, 3)].shape[0] == m.voxels()
            assert st["integrated"] == sum(_points(f[0]) for f in frames)
            if not lds:
                assert st["direct"] == st["integrated"]


# ------------------------------------------------------ 2 scalar load path --
@pytest.mark.parametrize("W,H", [(97, 53), (1, 300), (2049, 1)])
def test_ragged_and_narrow_frames_remove_one_of_two(W, H):
    a, b = _frame(W, H, W * 7 + H), _frame(W, H, W * 11 + H)
    rng = np.random.default_rng(W + H)
    Ta, Tb = _pose(rng), _pose(rng)
    with youth_map.VoxelMap(100.0, slots=1 << 16) as m:
        m.integrate(*a, T_world=Ta)
        m.integrate(*b, T_world=Tb)
        m.remove(*a, T_world=Ta)
        _same(m.extract(), restate(*frame_points(*b, None, Tb), 100.0)[0])
        _clean(m, removed=_points(a[0]))
        m.clear()
        m.integrate(a[0], None, T_world=Ta)
        m.integrate(b[0], None, T_world=Tb)
        m.remove(b[0], None, T_world=Tb)
        _same(m.extract(), restate(*frame_points(a[0], None, None, Ta), 100.0)[0])
        _clean(m, removed=_points(b[0]))


def test_device_pointers_offset_by_one_element():
    """Depth and colour misaligned by one element: the scalar loads of the
    removing kernel, on a torch stream."""
    W, H, n, vpm = 64, 48, 3, 100.0
    rng = np.random.default_rng(9)
    frames = [_frame(W, H, 300 + f) for f in range(n)]
    T = np.stack([_pose(rng) for _ in range(n)])
    b = _Batch(frames, T, range(n), offset=1)
    stream = torch.cuda.current_stream().cuda_stream
    with youth_map.VoxelMap(vpm, slots=1 << 16) as m:
        m.sync()
        m.integrate_device(*b.args(), stream=stream)
        m.remove_device(*b.args(1, 1), stream=stream)
        m.sync(stream)
        _same(m.extract(), restate_frames([(*frames[f], None, T[f]) for f in (0, 2)], vpm)[0])
        _clean(m, removed=_points(frames[1][0]))


# ------------------------------------------------------------ 3 contention --
def test_contention_wall_in_few_voxels_remove_one_of_two():
    """The wall of test_contention_wall_in_few_voxels: thousands of points per
    voxel, the LDS table summing many runs before one subtraction per slot."""
    W, H, vpm = 320, 240, 4.0
    rng = np.random.default_rng(1)
    walls = [(np.full((H, W), d, np.int16), rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8))
             for d in (2000, 2100)]
    want, _ = restate(*frame_points(*walls[0]), vpm)
    assert want.shape[0] <= 64 and want["count"].max() >= 2000
    with youth_map.VoxelMap(vpm, slots=4096) as m:
        m.integrate(*walls[0])
        m.integrate(*walls[1])
        assert int(m.extract()["count"].sum()) == 2 * W * H
        m.remove(*walls[1])
        _same(m.extract(), want)
        _clean(m, removed=W * H)


# -------------------------------------------- 4 remove everything, refill --
def test_remove_everything_and_refill_reuses_the_slots():
    frames, T, K, vpm, truth = _four()
    want = truth[True, (0, 1, 2, 3)]
    with youth_map.VoxelMap(vpm) as m:
        b = _integrate_four(m)
        a = b.args()
        occupied = m.stats()["occupied"]
        assert occupied == want.shape[0]
        m.remove_device(*a[:5], a[5], K)
        assert m.extract().shape == (0,)
        st, rs = _clean(m, removed=sum(_points(f[0]) for f in frames), vacant=occupied)
        assert rs["live"] == 0 and st["occupied"] == occupied == m.voxels()
        m.integrate_device(*a[:5], a[5], K)
        _same(m.extract(), want)
        st, rs = _clean(m, vacant=0)
        assert st["occupied"] == occupied and rs["live"] == occupied
    with youth_map.VoxelMap(vpm) as fresh:
        _integrate_four(fresh)
        _same(fresh.extract(), want)


# -------------------------------------------------------------- 5 max_depth --
def test_removal_uses_the_maps_max_depth():
    depth, rgb = _frame(97, 53, 500)
    T = _pose(np.random.default_rng(2))
    n = _points(depth, 9000)
    assert 0 < n < _points(depth)
    with youth_map.VoxelMap(100.0) as m:
        m.set_max_depth(9000)
        m.integrate(depth, rgb, T_world=T)
        _same(m.extract(), restate(*frame_points(depth, rgb, None, T, max_depth=9000), 100.0)[0])
        m.remove(depth, rgb, T_world=T)
        assert m.extract().shape == (0,)
        st, rs = _clean(m, removed=n, vacant=m.voxels())
        assert st["integrated"] == n and rs["live"] == 0


# ------------------------------------------------------------------ 6 misuse --
def test_misuse_is_counted_never_waited_for():
    a, b = _frame(97, 53, 12), _frame(97, 53, 13)
    far = np.array([[1, 0, 0, 500.0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float64)   # 500 m along x
    want, oor = restate(*frame_points(*a), 100.0)
    assert oor == 0 and restate(*frame_points(*b, None, far), 100.0)[1] == 0
    with youth_map.VoxelMap(100.0) as m:
        m.integrate(*a)
        m.remove(*b, T_world=far)                        # never integrated: no voxel of it exists
        rs = m.remove_stats()
        assert rs["missing"] == _points(b[0]) and rs["removed"] == 0 and rs["underflow"] == 0
        assert rs["vacant"] == rs["stale"] == 0
        _same(m.extract(), want)
        m.remove(*a)
        assert m.extract().shape == (0,) and m.remove_stats()["underflow"] == 0
        m.remove(*a)                                     # a second time: every count goes below zero
        rs = m.remove_stats()
        assert rs["underflow"] > 0 and rs["missing"] == _points(b[0])
        assert m.stats()["dropped"] == 0


# ------------------------------------------------------------- 7 compaction --
def test_compact_after_subset_removal():
    frames, T, K, vpm, truth = _four()
    want = truth[True, (0, 2)]
    views = [np.vstack([T[0], [0, 0, 0, 1]]).astype(np.float64), np.eye(4)]
    render = lambda m: [m.render(V, 160, 120, K) for V in views]
    with youth_map.VoxelMap(vpm) as m:
        b = _integrate_four(m)
        for f in (1, 3):
            a = b.args(f, 1)
            m.remove_device(*a[:5], a[5], K)
        _same(m.extract(), want)
        before = render(m)
        st0, rs0 = _clean(m)
        assert rs0["vacant"] > 0 and m.voxels() > want.shape[0]
        m.compact()
        _same(m.extract(), want)
        st1, rs1 = _clean(m, removed=rs0["removed"], vacant=0)
        assert m.voxels() == want.shape[0] == st1["occupied"] == rs1["live"]
        assert {k: v for k, v in st1.items() if k != "occupied"} == \
               {k: v for k, v in st0.items() if k != "occupied"}
        after = render(m)
        m.compact()                                      # nothing vacant: the same again
        _same(m.extract(), want)
    with youth_map.VoxelMap(vpm) as fresh:
        for f in (0, 2):
            fresh.integrate(*frames[f], K, T[f])
        _same(fresh.extract(), want)
        remaining = render(fresh)
    for (d0, c0), (d1, c1), (d2, c2) in zip(before, after, remaining):
        assert (d0 != 0).any()
        assert d0.tobytes() == d1.tobytes() == d2.tobytes()
        assert c0.tobytes() == c1.tobytes() == c2.tobytes()


# ------------------------------------------------------------------- 8 move --
@pytest.mark.parametrize("moved", [(0, 1, 2, 3), (1, 3)])
def test_move_device_from_perturbed_to_true_poses(moved):
    """Four frames integrated with perturbed poses and moved to the true ones:
    the map of a fresh integration with the true poses.  Frames whose poses are
    bitwise equal in the two arrays are skipped by both launches: `removed`
    counts the other frames' points only."""
    frames, T, K, vpm, truth = _four()
    T_old = T.copy()
    for f in moved:
        T_old[f, :, 3] += np.float32(0.013) * (f + 1)
    start, oor = restate_frames([(*frames[f], K, T_old[f]) for f in range(4)], vpm)
    assert oor == 0
    b = _Batch(frames, T_old, range(4))
    d_T_new = torch.from_numpy(np.ascontiguousarray(T).reshape(4, 12)).cuda()
    torch.cuda.synchronize()
    with youth_map.VoxelMap(vpm) as m:
        a = b.args()
        m.integrate_device(*a[:5], a[5], K)
        _same(m.extract(), start)
        m.move_device(*a[:5], a[5], d_T_new.data_ptr(), K)
        _same(m.extract(), truth[True, (0, 1, 2, 3)])
        n_moved = sum(_points(frames[f][0]) for f in moved)
        st, rs = _clean(m, removed=n_moved)
        assert st["integrated"] == sum(_points(f[0]) for f in frames) + n_moved
        m.move_device(*a[:5], d_T_new.data_ptr(), d_T_new.data_ptr(), K)   # nothing moves
        _same(m.extract(), truth[True, (0, 1, 2, 3)])
        _clean(m, removed=n_moved)
