"""The kernel instantiations of the side units that a host-side switch selects
and no other test file launches (profiles/variants/reach_parent.txt, DESIGN.md
§18): the rectifier's map-reading form, the viewer scan with more than one
tile per thread, the voxel map's [remove][vec][lds][rgb] cube and both legs of
a move, k_rgbd_pull at a forced grid, the renderer's per-lane splat loop in
this process.  Each against the truth its unit already
has, bit for bit: these units are integer work or IEEE as written, so nothing
here has a tolerance."""
import functools

import numpy as np
import pytest
import torch

import oracle
import youth_icp
import youth_map
import youth_rgbd
import youth_synth
import youth_viewer
from map_truth import restate_frames
from test_gpu_map_remove import _Batch, _clean, _points, _pose, _same
from test_gpu_map_remove import _frame as _map_frame
from test_gpu_rectify import make, on_device, planes, truth
from test_gpu_render import K_RAND, render, view_from_pose
from test_gpu_render import _same as _same_render
from test_gpu_rgbd_track import _host_frames
from test_gpu_viewer import _frame, check_guarded_vertices, guarded_vertices

pytestmark = pytest.mark.gpu


# ------------------------------------------- 1 rectifier, map-reading form --
@pytest.mark.parametrize("name", ["barrel160", "scalar162", "ragged97", "tiny2x2"])
def test_rectify_map_form_equals_truth_and_the_recomputing_form(name, monkeypatch):
    """YOUTH_RECTIFY_MAP=1 (read at create): k_rectify<vec, true> takes its map
    words from the stored map; scalar162 and ragged97 run the element stores and,
    on 97, lanes past the row's end (the map[in ? o + j : 0] guard).  Every
    output is the restatement's and byte-equal to the recomputing form's."""
    monkeypatch.setenv("YOUTH_RECTIFY_MAP", "1")
    stored = make(name)
    monkeypatch.setenv("YOUTH_RECTIFY_MAP", "0")
    recomputed = make(name)
    with stored, recomputed:
        # two frames with 3-channel colour, then the 1-channel plane alone
        d, c3, c1 = planes(name, 2)
        want_d, want_c3 = truth(name, d, c3)
        want_c1 = truth(name, None, c1)[1]
        got = [(on_device(r, d, c3), on_device(r, None, c1)[1]) for r in (stored, recomputed)]
        for (got_d, got_c3), got_c1 in got:
            assert np.array_equal(got_d, want_d) and np.array_equal(got_c3, want_c3)
            assert np.array_equal(got_c1, want_c1)
        assert got[0][0][0].tobytes() == got[1][0][0].tobytes()
        assert got[0][0][1].tobytes() == got[1][0][1].tobytes()
        assert got[0][1].tobytes() == got[1][1].tobytes()

        # bases one element past an aligned one, 77-filled guards around the outputs
        def shifted(a, off, fill):
            buf = torch.full((a.size + 16,), fill, dtype=torch.from_numpy(a).dtype, device="cuda")
            view = buf[off:off + a.size].view(a.shape)
            view.copy_(torch.from_numpy(a).cuda())
            return buf, view

        d, c3, c1 = planes(name, 2, seed=9)
        want_d, want_c3 = truth(name, d, c3)
        want_c1 = truth(name, None, c1)[1]
        for off_in, off_out in ((1, 0), (0, 1), (1, 1)):
            for c, want_c in ((c3, want_c3), (c1, want_c1)):
                outs = []
                for r in (stored, recomputed):
                    _, di = shifted(d, off_in, 0)
                    _, ci = shifted(c, off_in, 0)
                    dbuf, do = shifted(np.zeros_like(d), off_out, 77)
                    cbuf, co = shifted(np.zeros_like(c), off_out, 77)
                    assert di.data_ptr() % 8 == 2 * off_in and do.data_ptr() % 8 == 2 * off_out
                    r.device_frames(di, do, ci, co)
                    torch.cuda.synchronize()
                    outs.append((do.cpu().numpy(), co.cpu().numpy()))
                    assert np.array_equal(outs[-1][0], want_d) and np.array_equal(outs[-1][1], want_c)
                    for buf, size in ((dbuf, d.size), (cbuf, c.size)):
                        assert (buf[:off_out] == 77).all() and (buf[off_out + size:] == 77).all()
                assert outs[0][0].tobytes() == outs[1][0].tobytes()
                assert outs[0][1].tobytes() == outs[1][1].tobytes()

        # 65 frames in one call
        d, c3, _ = planes(name, 65, seed=65)
        want_d, want_c3 = truth(name, d, c3)
        outs = [on_device(r, d, c3) for r in (stored, recomputed)]
        for got_d, got_c in outs:
            assert np.array_equal(got_d, want_d) and np.array_equal(got_c, want_c3)
        assert outs[0][0].tobytes() == outs[1][0].tobytes()
        assert outs[0][1].tobytes() == outs[1][1].tobytes()
    if name != "tiny2x2":
        assert (want_d != d).any() and (want_d > 0).any()


# ------------------------------------- 2 viewer scan, R >= 2, guarded lists --
@pytest.mark.parametrize("W,H,px,tiles", [(1024, 513, 8, 257), (1024, 513, 4, 513), (1031, 509, 8, 257)],
                         ids=["1024x513_px8_R2", "1024x513_px4_R3", "1031x509_px8_R2_scalar"])
def test_cloud_scan_with_several_tiles_per_thread(W, H, px, tiles, monkeypatch):
    """More than 256 tiles: k_cloud_scan's thread owns R = 2 (3) consecutive
    tiles, at 257 tiles thread 128 owns one and the threads above none, and
    counts[f] comes from a thread that owns nothing.  A band of empty rows puts
    several empty tiles into one thread's run, the last tile is empty, the
    second frame is all zero."""
    monkeypatch.setenv("YOUTH_CLOUD_PX", str(px))
    N = W * H
    assert (N + 256 * px - 1) // (256 * px) == tiles > 256
    depth, rgb = _frame(W, H, W + px)
    depth[100:132] = 0
    depth.reshape(-1)[-3000:] = 0
    frames = [(depth, rgb), (np.zeros_like(depth), rgb)]
    rng = np.random.default_rng(px)
    T = np.stack([_pose(rng), _pose(rng, big=True)])
    d_all = torch.from_numpy(np.stack([f[0] for f in frames])).cuda()
    c_all = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
    d_T = torch.from_numpy(T.reshape(2, 12)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    with youth_viewer.CloudBuilder(W, H, max_frames=2) as cb:
        for posed in (False, True):
            verts = guarded_vertices(2, N)
            counts = torch.full((2,), -1, dtype=torch.int32, device="cuda")
            if posed:
                cb.build_device_posed(d_all.data_ptr(), c_all.data_ptr(), 2, W, H, d_T.data_ptr(),
                                      verts.data_ptr(), counts.data_ptr(), stream=stream)
            else:
                cb.build_device(d_all.data_ptr(), c_all.data_ptr(), 2, W, H, verts.data_ptr(),
                                counts.data_ptr(), stream=stream)
            torch.cuda.synchronize()
            wants = [oracle.viewer_cloud(d, c, T_world=T[f] if posed else None)
                     for f, (d, c) in enumerate(frames)]
            assert wants[0].shape[0] == int((depth > 0).sum()) > N // 2 and wants[1].shape[0] == 0
            check_guarded_vertices(verts.cpu().numpy(), counts.cpu().numpy(), wants, N)


# -------------------------------------------------- 3 voxel map, the cube --
MAP_FRAMES = {"64x48_vector": (64, 48, 0), "97x53_scalar": (97, 53, 0), "64x48_offset1_scalar": (64, 48, 1)}


@functools.lru_cache(maxsize=None)
def _map_case(kind):
    """Three frames, their poses, the new poses of frames 0 and 2, and per
    colour setting the restatement after each of the four steps."""
    W, H, offset = MAP_FRAMES[kind]
    vpm = 100.0
    rng = np.random.default_rng(W + offset)
    frames = [_map_frame(W, H, 700 + W + f) for f in range(3)]
    T = np.stack([_pose(rng) for _ in range(3)])
    Tn = np.stack([_pose(rng) for _ in range(3)])
    want = {}
    for colour in (True, False):
        fr = lambda f, P: (frames[f][0], frames[f][1] if colour else None, None, P[f])
        steps = [[fr(0, T), fr(1, T), fr(2, T)], [fr(0, T), fr(2, T)], [fr(0, Tn), fr(2, T)],
                 [fr(0, Tn), fr(2, Tn)]]
        for k, s in enumerate(steps):
            want[colour, k], oor = restate_frames(s, vpm)
            assert oor == 0
    return frames, T, Tn, vpm, want


@pytest.mark.parametrize("kind", sorted(MAP_FRAMES))
def test_map_cube_integrate_remove_and_both_legs_of_a_move(kind, monkeypatch):
    """k_map_integrate[vec][lds][rgb] and k_map_update[remove][vec][lds][rgb]:
    per frame kind (vec) the loop runs colour x YOUTH_MAP_LDS; removal runs the
    removing form, move_device the removing and the adding one.  64x48 is one
    and a half 2048-pixel tiles."""
    W, H, offset = MAP_FRAMES[kind]
    frames, T, Tn, vpm, want = _map_case(kind)
    pts = [_points(f[0]) for f in frames]
    all3 = _Batch(frames, T, range(3), offset=offset)
    # the frames that remain after the removal, at the poses before and after each move
    pair = _Batch(frames, T, (0, 2), offset=offset)
    T_step3 = torch.from_numpy(np.ascontiguousarray(np.stack([Tn[0], T[2]])).reshape(2, 12)).cuda()
    T_step4 = torch.from_numpy(np.ascontiguousarray(np.stack([Tn[0], Tn[2]])).reshape(2, 12)).cuda()
    torch.cuda.synchronize()
    assert (all3.args()[0] % 16 == 0 and W * H % 8 == 0) == (kind == "64x48_vector")
    for lds in (1, 0):
        monkeypatch.setenv("YOUTH_MAP_LDS", str(lds))
        with youth_map.VoxelMap(vpm, slots=1 << 18) as m:
            for colour in (True, False):
                m.clear()
                a = all3.args(colour=colour)
                m.integrate_device(*a)
                _same(m.extract(), want[colour, 0])
                _clean(m, removed=0, vacant=0)
                a = all3.args(1, 1, colour)
                m.remove_device(*a)
                _same(m.extract(), want[colour, 1])
                _clean(m, removed=pts[1])
                # frame 0 alone to its new pose
                a = pair.args(0, 1, colour)
                m.move_device(*a[:5], a[5], T_step3.data_ptr())
                _same(m.extract(), want[colour, 2])
                _clean(m, removed=pts[1] + pts[0])
                # frames 0 and 2: frame 0's pose is bitwise the same in both arrays
                a = pair.args(0, 2, colour)
                m.move_device(*a[:5], T_step3.data_ptr(), T_step4.data_ptr())
                _same(m.extract(), want[colour, 3])
                st, rs = _clean(m, removed=pts[1] + pts[0] + pts[2])
                assert st["integrated"] == sum(pts) + pts[0] + pts[2]
                assert rs["live"] == want[colour, 3].shape[0]
                if not lds:
                    assert st["direct"] == st["integrated"]
                else:
                    assert st["direct"] < st["integrated"]


# ------------------------------------------ 4 k_rgbd_pull at a forced grid --
@pytest.mark.parametrize("W,H", [(24, 16), (97, 53), (160, 120)])
@pytest.mark.parametrize("wg", [1, 7, 1024])
def test_pull_at_a_forced_grid_equals_numpy(wg, W, H, monkeypatch):
    """YOUTH_RGBD_PULL_WG (read at create).  At 160x120 (2400 depth vectors, 1200
    colour units) a grid of 1 runs the four-deep depth body nine times and its
    tail, a grid of 7 (stride 448) once and its tail, a grid of 1024 leaves
    most lanes without work.  Assertions and guards of test_pull_equals_numpy."""
    monkeypatch.setenv("YOUTH_RGBD_PULL_WG", str(wg))
    rng = np.random.default_rng(W * 3 + wg)
    N, PAD = W * H, 64
    depth = rng.integers(-32768, 32768, (8, H, W)).astype(np.int16)
    rgb = rng.integers(0, 256, (8, H, W, 3), dtype=np.uint8)
    rgb[:, 0, :4] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 0, 255]]
    Y = youth_synth.luma(rgb)
    with youth_rgbd.RgbdContext(W, H, 2) as ctx:
        for kind in ("pinned", "pageable", "offset"):
            dl, cl, bufs = _host_frames(depth, rgb, kind)
            for m in (1, 8):
                for want_rgb in (False, True):
                    d_d = torch.full((m * N + PAD,), -7, dtype=torch.int16, device="cuda")
                    d_g = torch.full((m * N + PAD,), 9, dtype=torch.uint8, device="cuda")
                    d_c = torch.full((m * N * 3 + PAD,), 5, dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    ctx.pull_host(dl[:m], cl[:m], d_d, d_g, d_c if want_rgb else None)
                    ctx.sync()
                    got_d, got_g, got_c = d_d.cpu().numpy(), d_g.cpu().numpy(), d_c.cpu().numpy()
                    assert np.array_equal(got_d[:m * N], depth[:m].reshape(-1)), (kind, m, want_rgb)
                    assert np.array_equal(got_g[:m * N], Y[:m].reshape(-1)), (kind, m, want_rgb)
                    assert (got_d[m * N:] == -7).all() and (got_g[m * N:] == 9).all()
                    if want_rgb:
                        assert np.array_equal(got_c[:m * N * 3], rgb[:m].reshape(-1)), (kind, m)
                        assert (got_c[m * N * 3:] == 5).all()
                    else:
                        assert (got_c == 5).all()
            for b in bufs:
                b.close()


# --------------------------------- 5 map render, the per-lane splat loop --
def test_render_loop_splat_path_equals_truth(monkeypatch):
    """YOUTH_MAP_RENDER_QUEUE=0 (read at the map's create): k_map_render_splat<false>,
    in this process; tests/test_gpu_render.py runs it in a child.  The child's
    recipe: two 160x120 frames, a full view and a 40x30 one clamped to 2 px."""
    monkeypatch.setenv("YOUTH_MAP_RENDER_QUEUE", "0")
    K = youth_icp.Intrinsics(*K_RAND)
    rng = np.random.default_rng(4)
    with youth_map.VoxelMap(100.0, slots=1 << 16) as m:
        for f in range(2):
            d, c = _map_frame(160, 120, 900 + f)
            m.integrate(d, c, K, _pose(rng))
        T = np.vstack([_pose(rng), [0, 0, 0, 1]]).astype(np.float64)
        rec = m.extract()
        full = m.render(T, 160, 120, K)
        small = m.render(T, 40, 30, K, max_splat=2)
        again = m.render(T, 160, 120, K)
    V = view_from_pose(T)
    want = render(rec, 100.0, V, K, 160, 120)
    assert (want[0] > 0).sum() > 1000
    _same_render(full, want)
    _same_render(again, want)
    _same_render(small, render(rec, 100.0, V, K, 40, 30, 2))
