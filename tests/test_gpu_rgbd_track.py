"""The streaming RGB-D tracker on the GPU (include/youth_rgbd.h, DESIGN.md
§14): the ingest kernel k_rgbd_pull against numpy, the tracker against the
sequence align it streams (youth_rgbd_track_host_sequence), its independence of
how a sequence is split into submissions, the depth filter in front of it and
its protocol."""
import ctypes
import os

import numpy as np
import pytest
import torch

import youth_filter
import youth_icp
import youth_rgbd
import youth_synth

pytestmark = pytest.mark.gpu

E = youth_icp.YOUTH_EINVAL


class _Pinned:
    """A youth_icp_host_alloc buffer of nbytes as a uint8 view."""

    def __init__(self, nbytes):
        self._lib = youth_icp.load_library()
        self.ptr = self._lib.youth_icp_host_alloc((nbytes + 1) // 2)
        assert self.ptr
        self.u8 = np.ctypeslib.as_array(ctypes.cast(self.ptr, ctypes.POINTER(ctypes.c_uint8)),
                                        shape=(nbytes,))

    def close(self):
        if self.ptr:
            self.u8 = None
            self._lib.youth_icp_host_free(self.ptr)
            self.ptr = None


def _host_frames(depth, rgb, kind):
    """The frames as lists of host arrays of `kind`: pageable, pinned, or pinned
    and offset by one element (int16 for depth, byte for colour).  Returns
    (depth list, rgb list, buffers to close)."""
    if kind == "pageable":
        return [np.ascontiguousarray(d) for d in depth], [np.ascontiguousarray(c) for c in rgb], []
    off = 1 if kind == "offset" else 0
    dl, cl, bufs = [], [], []
    for d, c in zip(depth, rgb):
        H, W = d.shape
        bd, bc = _Pinned((d.size + off) * 2), _Pinned(c.size + off)
        dv = bd.u8[2 * off:2 * (off + d.size)].view(np.int16).reshape(H, W)
        cv = bc.u8[off:off + c.size].reshape(H, W, 3)
        dv[:] = d
        cv[:] = c
        assert dv.ctypes.data % 16 == 2 * off and cv.ctypes.data % 16 == off
        dl.append(dv)
        cl.append(cv)
        bufs += [bd, bc]
    return dl, cl, bufs


# ------------------------------------------------------------- pull kernel --
@pytest.mark.parametrize("kind", ["pinned", "pageable", "offset"])
@pytest.mark.parametrize("W,H", [(24, 16), (97, 53), (160, 120)])
def test_pull_equals_numpy(W, H, kind):
    rng = np.random.default_rng(W * 3 + len(kind))
    N, PAD = W * H, 64
    depth = rng.integers(-32768, 32768, (8, H, W)).astype(np.int16)
    rgb = rng.integers(0, 256, (8, H, W, 3), dtype=np.uint8)
    rgb[:, 0, :4] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 0, 255]]
    Y = youth_synth.luma(rgb)
    dl, cl, bufs = _host_frames(depth, rgb, kind)
    with youth_rgbd.RgbdContext(W, H, 2) as ctx:
        for m in (1, 3, 8):
            for want_rgb in (False, True):
                d_d = torch.full((m * N + PAD,), -7, dtype=torch.int16, device="cuda")
                d_g = torch.full((m * N + PAD,), 9, dtype=torch.uint8, device="cuda")
                d_c = torch.full((m * N * 3 + PAD,), 5, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                ctx.pull_host(dl[:m], cl[:m], d_d, d_g, d_c if want_rgb else None)
                ctx.sync()
                got_d, got_g, got_c = d_d.cpu().numpy(), d_g.cpu().numpy(), d_c.cpu().numpy()
                assert np.array_equal(got_d[:m * N], depth[:m].reshape(-1)), (m, want_rgb)
                assert np.array_equal(got_g[:m * N], Y[:m].reshape(-1)), (m, want_rgb)
                assert (got_d[m * N:] == -7).all() and (got_g[m * N:] == 9).all()
                if want_rgb:
                    assert np.array_equal(got_c[:m * N * 3], rgb[:m].reshape(-1)), m
                    assert (got_c[m * N * 3:] == 5).all()
                else:
                    assert (got_c == 5).all()
    for b in bufs:
        b.close()


# -------------------------------------------------------- tracker helpers --
def _track(ctx, depth, rgb, split):
    """Stream the frames in submissions of the given sizes, two in flight."""
    T, has, st = [], [], []
    sizes = []

    def collect():
        for _ in range(sizes.pop(0)):
            t, h, s = ctx.track_collect()
            T.append(t)
            has.append(h)
            st.append(s)

    f = 0
    for m in split:
        if len(sizes) == 2:
            collect()
        ctx.track_submit(depth[f:f + m], rgb[f:f + m])
        sizes.append(m)
        f += m
    while sizes:
        collect()
    assert f == len(depth) and ctx.track_pending() == 0
    return np.array(T), np.array(has), np.array(st)


@pytest.fixture(scope="module")
def seq160():
    depth, _, rgb = youth_synth.sequence_rgb(0, 9, 160, 120)
    return list(depth), list(rgb), depth, rgb


SPLITS = ([1] * 9, [1, 8], [3, 3, 3], [8, 1])


def _splits_agree(seq160, lam=0.1):
    dl, cl, depth, rgb = seq160
    runs = []
    for split in SPLITS:
        with youth_rgbd.RgbdContext(160, 120, 16, lam=lam) as ctx:
            assert ctx.track_set_batch(8) == 1
            runs.append(_track(ctx, dl, cl, split))
    T, has, st = runs[0]
    assert has.tolist() == [0] + [1] * 8 and np.array_equal(T[0], np.eye(4))
    for Tk, hk, sk in runs[1:]:
        assert np.array_equal(Tk, T) and np.array_equal(hk, has) and np.array_equal(sk, st)
    with youth_rgbd.RgbdContext(160, 120, 16, lam=lam) as ctx:
        Tseq, stseq = ctx.track_host_sequence(depth, rgb)
    Tseq[:, 3, :] = (0.0, 0.0, 0.0, 1.0)
    return T[1:], st[1:], Tseq, stseq


# ------------------------------------------------------ split independence --
def test_splits_are_bit_identical_and_equal_the_sequence(seq160, monkeypatch):
    """The same kernels on the same geometry and records give the same bits."""
    monkeypatch.setenv("YOUTH_RGBD_CHUNKS", "7")
    T, st, Tseq, stseq = _splits_agree(seq160)
    assert np.array_equal(T, Tseq) and np.array_equal(st, stseq)
    assert (st == 0).all()


def test_splits_without_the_knob_within_launch_shape_bar(seq160, monkeypatch):
    monkeypatch.delenv("YOUTH_RGBD_CHUNKS", raising=False)
    T, st, Tseq, stseq = _splits_agree(seq160)
    print("max |T - T_seq|:", np.abs(T - Tseq).max())
    assert np.abs(T - Tseq).max() <= 1e-9 and np.array_equal(st, stseq)


def test_odd_size_batch_one_lambda_zero(monkeypatch):
    monkeypatch.delenv("YOUTH_RGBD_CHUNKS", raising=False)
    depth, _, rgb = youth_synth.sequence_rgb(0, 5, 97, 53)
    with youth_rgbd.RgbdContext(97, 53, 4, lam=0.0) as ctx:
        assert ctx.track_set_batch(1) == 1
        T, has, st = _track(ctx, list(depth), list(rgb), [1] * 5)
    with youth_rgbd.RgbdContext(97, 53, 4, lam=0.0) as ctx:
        Tseq, stseq = ctx.track_host_sequence(depth, rgb)
    Tseq[:, 3, :] = (0.0, 0.0, 0.0, 1.0)
    assert has.tolist() == [0, 1, 1, 1, 1]
    print("max |T - T_seq|:", np.abs(T[1:] - Tseq).max())
    assert np.abs(T[1:] - Tseq).max() <= 1e-9 and np.array_equal(st[1:], stseq)


# ------------------------------------------------------------ depth filter --
def test_depth_filter_equals_prefiltered_frames(seq160):
    dl, cl, depth, _ = seq160
    filtered = list(youth_filter.depth_filter_host(depth[:6], 8, 96))
    assert any(not np.array_equal(a, b) for a, b in zip(filtered, dl))
    with youth_rgbd.RgbdContext(160, 120, 16) as ctx:
        ctx.track_set_batch(4)
        ctx.track_set_depth_filter(8, 96)
        on = _track(ctx, dl[:6], cl[:6], [2, 4])
        ctx.track_reset()
        ctx.track_set_depth_filter(None)
        off = _track(ctx, filtered, cl[:6], [2, 4])
    for a, b in zip(on, off):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- protocol --
def test_protocol_and_refusals(seq160):
    dl, cl, _, _ = seq160
    with youth_rgbd.RgbdContext(160, 120, 8) as ctx:
        lib, h = ctx._lib, ctx._ctx
        err = lambda: (lib.youth_rgbd_last_error() or b"").decode()
        assert ctx.track_set_batch(4) == 1
        want = _track(ctx, dl[:6], cl[:6], [2, 4])
        assert want[1].tolist() == [0, 1, 1, 1, 1, 1] and np.array_equal(want[0][0], np.eye(4))
        ctx.track_reset()

        T = np.zeros(16)
        Tp = T.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        has = ctypes.c_int()
        VP = ctypes.c_void_p
        good_d = (VP * 8)(*[a.ctypes.data for a in dl[:8]])
        good_c = (VP * 8)(*[a.ctypes.data for a in cl[:8]])
        hole_d = (VP * 8)(*[a.ctypes.data for a in dl[:8]])
        hole_d[1] = None
        hole_c = (VP * 8)(*[a.ctypes.data for a in cl[:8]])
        hole_c[1] = None
        idle = {
            "collect nothing pending": lambda: lib.youth_rgbd_track_collect(h, Tp, ctypes.byref(has)),
            "submit 0 frames": lambda: lib.youth_rgbd_track_submit(h, good_d, good_c, 0),
            "submit above b": lambda: lib.youth_rgbd_track_submit(h, good_d, good_c, 5),
            "submit null depth": lambda: lib.youth_rgbd_track_submit(h, hole_d, good_c, 2),
            "submit null colour": lambda: lib.youth_rgbd_track_submit(h, good_d, hole_c, 2),
            "submit null arrays": lambda: lib.youth_rgbd_track_submit(h, None, None, 1),
            "set_batch 0": lambda: lib.youth_rgbd_track_set_batch(h, 0),
            "set_batch beyond max_frames / 2": lambda: lib.youth_rgbd_track_set_batch(h, 5),
        }
        for name, call in idle.items():
            assert call() == E, name
            assert "youth_rgbd_track" in err(), (name, err())
        # two submissions in flight are accepted, a third is refused; so are
        # set_batch, reset and the filter switch while frames are pending
        ctx.track_submit(dl[:2], cl[:2])
        ctx.track_submit(dl[2:6], cl[2:6])
        busy = {
            "third submission": lambda: lib.youth_rgbd_track_submit(h, good_d, good_c, 1),
            "set_batch with frames pending": lambda: lib.youth_rgbd_track_set_batch(h, 2),
            "reset with frames pending": lambda: lib.youth_rgbd_track_reset(h),
            "filter with frames pending": lambda: lib.youth_rgbd_track_set_depth_filter(h, None),
        }
        for name, call in busy.items():
            assert call() == E, name
            assert "youth_rgbd_track" in err(), (name, err())
        assert ctx.track_pending() == 6
        got = [ctx.track_collect() for _ in range(6)]
        for k in range(6):
            assert np.array_equal(got[k][0], want[0][k]) and got[k][1] == want[1][k] \
                and got[k][2] == want[2][k]
        # after every refusal the context tracks bit for bit as before
        ctx.track_reset()
        again = _track(ctx, dl[:6], cl[:6], [2, 4])
        for a, b in zip(again, want):
            assert np.array_equal(a, b)
    with youth_rgbd.RgbdContext(160, 120, 8) as ctx:
        with pytest.raises(youth_icp.IcpError) as e:
            ctx.track_set_batch(5)
        assert e.value.code == E and "max_frames" in str(e.value)
