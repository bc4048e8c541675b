"""GPU tests of the lens rectifier (include/youth_rectify.h):
k_rectify_map and k_rectify against the numpy restatement bit for bit: the
maps of the cameras, depth and colour applies on both store paths and on odd
bases, every plane selection, frame count and entry point, the identity at
D = 0, and the argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import rectify_truth as rt
import youth_icp
import youth_rectify
from test_rectify import CAMERAS, D_BARREL, K160, hostile_depth, intr

pytestmark = pytest.mark.gpu

APPLY = dict(CAMERAS)
APPLY["scalar162"] = (162, 120, K160, D_BARREL, None)     # W % 4 != 0: element stores


def make(name):
    W, H, K, D, Ko = APPLY[name]
    return youth_rectify.Rectifier(W, H, intr(K), D, None if Ko is None else intr(Ko))


def step_depth(W, H):
    """Row bands at 500 mm, 2 m and 8 m (the 255 cap) whose adjacent columns
    step by T - 1, T and T + 1: both sides of the gate."""
    d = np.zeros((H, W), np.int16)
    bands = [(n, s) for n in (500, 2000, 8000) for s in (-1, 0, 1)]
    odd = (np.arange(W) & 1).astype(np.int64)
    for k, (n, s) in enumerate(bands):
        T = int(rt.gate(n))
        lo, hi = k * H // len(bands), (k + 1) * H // len(bands)
        d[lo:hi] = (n + odd * (T + s)).astype(np.int16)[None, :]
    return d


def planes(name, n, seed=0):
    W, H = APPLY[name][:2]
    rng = np.random.default_rng(seed)
    d = np.stack([hostile_depth(W, H, seed + f) if f % 2 == 0 else step_depth(W, H) for f in range(n)])
    c3 = rng.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)
    c1 = rng.integers(0, 256, size=(n, H, W, 1), dtype=np.uint8)
    return d, c3, c1


def truth(name, d, c):
    W, H, K, D, Ko = APPLY[name]
    return rt.rectify(d, c, W, H, K, D, Ko)


def on_device(r, d, c):
    td = None if d is None else torch.from_numpy(d).cuda()
    tc = None if c is None else torch.from_numpy(c).cuda()
    od, oc = r.device_frames(td, None, tc, None)
    torch.cuda.synchronize()
    return (None if od is None else od.cpu().numpy()), (None if oc is None else oc.cpu().numpy())


# -------------------------------------------------------------------- maps --

@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_map_bit_exact(name):
    W, H, K, D, Ko = CAMERAS[name]
    with make(name) as r:
        got = r.map()
        assert got.dtype == np.uint32 and got.shape == (H, W, 2)
        assert np.array_equal(got, rt.map_words(W, H, K, D, Ko))
        assert r.covered == rt.covered_count(W, H, K, D, Ko)


# ----------------------------------------------------------------- applies --

@pytest.mark.parametrize("name", sorted(APPLY))
def test_apply_bit_exact_on_every_entry_point(name):
    """Two frames (hostile depth, gate steps) with 3-channel colour, then the
    1-channel plane alone: device, host in place and host_frames agree with
    the restatement."""
    d, c3, c1 = planes(name, 2)
    want_d, want_c3 = truth(name, d, c3)
    want_c1 = truth(name, None, c1)[1]
    if name in ("barrel160", "scalar162"):
        assert (want_d != d).any() and (want_d[1] > 0).any()
    with make(name) as r:
        got_d, got_c = on_device(r, d, c3)
        assert got_d.dtype == np.int16 and np.array_equal(got_d, want_d)
        assert got_c.dtype == np.uint8 and np.array_equal(got_c, want_c3)
        assert np.array_equal(on_device(r, None, c1)[1], want_c1)
        hd, hc = d.copy(), c3.copy()
        r.host(hd, hc, in_place=True)
        assert np.array_equal(hd, want_d) and np.array_equal(hc, want_c3)
        od, oc = r.host(d, c1)
        assert np.array_equal(od, want_d) and np.array_equal(oc, want_c1)
        fd, fc = [f.copy() for f in d], [f.copy() for f in c3]
        r.host_frames(fd, fc)
        assert np.array_equal(np.stack(fd), want_d) and np.array_equal(np.stack(fc), want_c3)
        fd = [f.copy() for f in d]
        r.host_frames(fd)
        assert np.array_equal(np.stack(fd), want_d)


@pytest.mark.parametrize("n", [1, 3, 65])
def test_apply_plane_selection_and_frame_counts(n):
    """Depth only, colour only and both, 1, 3 and 65 frames per call."""
    name = "barrel160"
    d, c3, _ = planes(name, n, seed=n)
    want_d, want_c = truth(name, d, c3)
    with make(name) as r:
        for dd, cc in ((d, None), (None, c3), (d, c3)):
            got_d, got_c = on_device(r, dd, cc)
            assert (got_d is None) == (dd is None) and (got_c is None) == (cc is None)
            assert dd is None or np.array_equal(got_d, want_d)
            assert cc is None or np.array_equal(got_c, want_c)
        hd, hc = r.host(d, c3)
        assert np.array_equal(hd, want_d) and np.array_equal(hc, want_c)
        assert np.array_equal(r.host(d)[0], want_d) and np.array_equal(r.host(None, c3)[1], want_c)
        fd, fc = [f.copy() for f in d], [f.copy() for f in c3]
        r.host_frames(fd, fc)
        assert np.array_equal(np.stack(fd), want_d) and np.array_equal(np.stack(fc), want_c)


@pytest.mark.parametrize("off_in,off_out", [(1, 0), (0, 1), (1, 1)])
def test_apply_on_bases_offset_by_one_element(off_in, off_out):
    """W = 160 with the inputs, the outputs or both one element past an aligned
    base: odd tap addresses under the vector stores, and the element stores."""
    name = "barrel160"
    W, H = APPLY[name][:2]
    d, c3, c1 = planes(name, 2, seed=9)
    want_d, want_c3 = truth(name, d, c3)
    want_c1 = truth(name, None, c1)[1]

    def shifted(a, off, fill):
        buf = torch.full((a.size + 16,), fill, dtype=torch.from_numpy(a).dtype, device="cuda")
        view = buf[off:off + a.size].view(a.shape)
        view.copy_(torch.from_numpy(a).cuda())
        return buf, view

    with make(name) as r:
        for c, want_c in ((c3, want_c3), (c1, want_c1)):
            _, di = shifted(d, off_in, 0)
            _, ci = shifted(c, off_in, 0)
            dbuf, do = shifted(np.zeros_like(d), off_out, 77)
            cbuf, co = shifted(np.zeros_like(c), off_out, 77)
            assert di.data_ptr() % 8 == 2 * off_in and do.data_ptr() % 8 == 2 * off_out
            r.device_frames(di, do, ci, co)
            torch.cuda.synchronize()
            assert np.array_equal(do.cpu().numpy(), want_d) and np.array_equal(co.cpu().numpy(), want_c)
            # nothing outside the outputs was written
            for buf, size in ((dbuf, d.size), (cbuf, c.size)):
                assert (buf[:off_out] == 77).all() and (buf[off_out + size:] == 77).all()


@pytest.mark.parametrize("name", ["barrel160", "scalar162", "ragged97", "tiny2x2"])
def test_no_distortion_returns_the_input(name):
    W, H, K = APPLY[name][:3]
    d, c3, c1 = planes(name, 2, seed=4)
    with youth_rectify.Rectifier(W, H, intr(K), (0, 0, 0, 0, 0)) as r:
        assert r.covered == W * H
        m = r.map()
        assert not (m[:H - 1, :W - 1, 0] & 0xFFF).any() and (m[..., 0] >> 31).all()
        got_d, got_c = on_device(r, d, c3)
        assert np.array_equal(got_d, d) and np.array_equal(got_c, c3)
        assert np.array_equal(on_device(r, None, c1)[1], c1)
        hd, hc = r.host(d, c3)
        assert np.array_equal(hd, d) and np.array_equal(hc, c3)


def test_bad_arguments_then_a_valid_call():
    name = "barrel160"
    W, H = APPLY[name][:2]
    d, c3, _ = planes(name, 1, seed=2)
    want_d, want_c = truth(name, d, c3)
    lib = youth_rectify.load_library()
    K = intr(K160)
    td, tc = torch.from_numpy(d).cuda(), torch.from_numpy(c3).cuda()
    od, oc = torch.empty_like(td), torch.empty_like(tc)
    two = torch.zeros(2 * d.size, dtype=torch.int16, device="cuda")
    c2 = torch.zeros((1, H, W, 2), dtype=torch.uint8, device="cuda")
    with make(name) as r:
        h = r._h
        raw = lib.youth_rectify_device
        cases = [
            lambda: r.device_frames(td, td),                                              # the same buffer
            lambda: r.device_frames(two[:d.size].view(d.shape), two[10:10 + d.size].view(d.shape)),
            lambda: r.device_frames(td, od, tc, tc),
            lambda: youth_rectify._check(lib, raw(h, td.data_ptr(), None, None, None, 3, 1, None)),   # half a pair
            lambda: youth_rectify._check(lib, raw(h, None, None, tc.data_ptr(), None, 3, 1, None)),
            lambda: youth_rectify._check(lib, raw(h, None, None, None, None, 3, 1, None)),            # no pair
            lambda: r.device_frames(None, None, c2),                                                  # channels = 2
            lambda: r.host(None, np.zeros((H, W, 2), np.uint8)),
            lambda: youth_rectify._check(lib, raw(h, td.data_ptr(), od.data_ptr(), None, None, 3, -1, None)),
            lambda: youth_rectify._check(lib, lib.youth_rectify_map_device(h, None, None)),
            lambda: youth_rectify.Rectifier(W, H, K, D_BARREL, intr((100.0, 100.0, 80.0, 60.0, 5000.0))),
            lambda: youth_rectify.Rectifier(W, H, K, (float("nan"), 0, 0, 0, 0)),
            lambda: youth_rectify.Rectifier(1, H, K, D_BARREL),
        ]
        for k, call in enumerate(cases):
            with pytest.raises(youth_icp.IcpError) as e:
                call()
            assert e.value.code == youth_icp.YOUTH_EINVAL, k
            assert (lib.youth_rectify_last_error() or b"").decode().strip(), k
        r.device_frames(td, od, tc, oc)
        torch.cuda.synchronize()
        assert np.array_equal(od.cpu().numpy(), want_d) and np.array_equal(oc.cpu().numpy(), want_c)
        hd, hc = r.host(d, c3)
        assert np.array_equal(hd, want_d) and np.array_equal(hc, want_c)
    assert isinstance(h, ctypes.c_void_p)
