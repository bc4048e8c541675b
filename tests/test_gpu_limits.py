"""The side units at the frame, batch and table limits they accept
(hip_host.h: W, H <= 16384, W * H <= 2^26, 65535 frames on gridDim.y, map
tables from 64 slots), each against its existing truth module, bit for bit;
every output element of every case is compared.

A  the largest and most extreme frames, one frame per call;
B  batches whose last frame starts at or past byte 2^32 of the call's largest
   array (the smallest such batch; all frames but the first and the last two
   identical, those four kinds different, so a wrapped offset meets other data);
C  65535 frames (the limit of gridDim.y) of the unit's smallest frame in one
   device call, every frame different; 65536 is refused and writes nothing;
D  the voxel map's extreme keys, its smallest table and the renderer's queue
   with all 1024 entries of a tile alive.

The inputs come from tests/limit_frames.py, whose constructions and counters
test_limits.py pins without a GPU.  Expected frames of 2^26 pixels are expanded
and compared on the device; the host sees them only to report a mismatch.

The rectifier's distorted apply runs in full on the strips 16384 x 2,
2 x 16384 and 16384 x 64; at 8192 x 8192 its map words are compared under the
barrel camera (the costliest numpy truth of the file), and its apply under the
no-distortion camera, where the output is the input, in the recomputing and
the map-reading form.  The viewer cloud also runs 8191 x 8193 (2^26 - 1 pixels:
the scalar loads and a partial last tile).  The map's boundary points travel
as one 1 x 1 frame each in one integrate call: a single frame's points are an
affine image of integer pixels and depths and cannot hold two neighbouring
fp32 values on one axis.

No test holds more than 10 GiB of device memory, the library's own buffers
included, at the points where `_memory_cap` samples it (the largest sample
is 9.1 GiB; the temporaries between samples are below 0.7 GiB).  Left out for that cap: RGB-D and ICP contexts over
17 and more frames of 2^26 pixels (their records are 1 GiB a frame), so no
RGB-D batch crosses 2^32 bytes; the RGB-D sums and the align against the numpy
truth run on 16384 x 48 and 48 x 16384 only.
"""
import numpy as np
import pytest
import torch

import filter_truth as ft
import limit_frames as lf
import loop_truth
import map_truth
import oracle
import rectify_truth
import render_truth
import rgbd_levels_truth
import rgbd_truth
import youth_filter
import youth_icp
import youth_loop
import youth_map
import youth_rectify
import youth_rgbd
import youth_synth
import youth_viewer
from test_gpu_rgbd import _poses3
from test_gpu_viewer import GUARD, NAN_BITS, guarded_vertices

pytestmark = pytest.mark.gpu

GIB = 1 << 30
CAP = 10 * GIB


class _Memory:
    """Device memory in use beyond what the test found, sampled where a test
    calls mark() (its inputs, outputs and the library's buffers live) and at
    teardown: a sample, not a true peak; a temporary between two marks (an
    index tensor, a gathered frame) is not seen."""

    def __init__(self):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        self.free0 = torch.cuda.mem_get_info()[0]
        self.peak = 0

    def mark(self):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()          # what torch only caches is not in use
        self.peak = max(self.peak, self.free0 - torch.cuda.mem_get_info()[0])
        return self.peak


@pytest.fixture(autouse=True)
def _memory_cap(request):
    mem = _Memory()
    request.node.limits_memory = mem
    yield mem
    mem.mark()
    print(f"sampled device memory: {mem.peak / (1 << 20):.0f} MiB  {request.node.name}")
    torch.cuda.empty_cache()
    assert mem.peak <= CAP, f"{mem.peak / GIB:.2f} GiB of device memory"


def _where(got, want):
    """The first differing elements, for the report of a failed torch.equal."""
    g, w = got.reshape(-1), want.reshape(-1)
    bad = torch.nonzero(g != w)[:5, 0].cpu().numpy()
    return [(int(i), int(g[i]), int(w[i])) for i in bad]


def _assert_equal(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if not torch.equal(got, want):
        raise AssertionError(f"{what}: (flat index, got, want) {_where(got, want)}")


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ready():
    """torch's fills and copies are complete: the cloud builder, the map and
    the RGB-D context run on streams of their own, which do not wait for
    torch's."""
    torch.cuda.synchronize()


# ================================================================ depth filter ==

FLT_B, FLT_HALO = 100, 2      # 100 rows: the repeats meet the 16-row tiles at 4 phases


def _filter_expected(block, H, phase, interior=None):
    """The expected frame of a periodic input, on the device."""
    if H < FLT_B + 2 * FLT_HALO:
        return _cuda(ft.filter_truth(lf.periodic_frame(block, H, phase), 8, 96))
    parts = lf.periodic_truth(lambda r: ft.filter_truth(r, 8, 96), block, H, FLT_HALO, phase, interior)
    rows = _cuda(lf.periodic_rows(H, FLT_B, phase))
    return lf.expand(*[_cuda(p) for p in parts], H, phase, index=rows)


def _periodic_on_device(block_d, H, phase):
    return block_d[_cuda(lf.periodic_rows(H, block_d.shape[0], phase))]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "base+2B"])
@pytest.mark.parametrize("shape", lf.shapes(3), ids=lf.shape_id)
def test_filter_largest_frames(shape, offset, _memory_cap):
    """A: both load paths (an 8-byte aligned base: short4 words; a base 2 bytes
    off: element loads) on 8192 x 8192, 16384 x 4096, 4096 x 16384, 16384 x 3
    and 3 x 16384."""
    W, H = shape
    assert lf.admitted(W, H, 3)
    block = lf.depth_block(FLT_B, W, 11 + W)
    want = _filter_expected(block, H, 5)
    buf = torch.zeros(H * W + 8, dtype=torch.int16, device="cuda")
    d_in = buf[offset:offset + H * W].view(H, W)
    d_in.copy_(_periodic_on_device(_cuda(block), H, 5))
    assert d_in.data_ptr() % 8 == 2 * offset
    obuf = torch.full((H * W + 8,), 0x5A5A, dtype=torch.int16, device="cuda")
    d_out = obuf[offset:offset + H * W].view(H, W)
    youth_filter.depth_filter_device(d_in, d_out, 8, 96)
    _memory_cap.mark()                                  # input, output and expected frame live
    _assert_equal(d_out, want, f"filter {W}x{H}")
    assert int((want != d_in).sum()) > H * W // 8          # the filter did filter
    assert (obuf[:offset] == 0x5A5A).all() and (obuf[offset + H * W:] == 0x5A5A).all()


def test_filter_batch_past_4_gib_33x8192x8192(_memory_cap):
    """B: 33 frames of 2^26 pixels; frame 32 starts at byte 2^32 of the input
    and of the output."""
    W, H, n = 8192, 8192, lf.smallest_batch_past_32_bits(2 * lf.MAX_PIXELS)
    assert n == 33 and lf.last_frame_offset(n, 2 * W * H) >= 1 << 32
    block = lf.depth_block(FLT_B, W, 3)
    block_d = _cuda(block)
    kinds, phases = lf.batch_kinds(n), (0, 7, 13, 29)
    d_in = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
    for f in range(n):
        d_in[f] = _periodic_on_device(block_d, H, phases[kinds[f]])
    d_out = torch.full((n, H, W), 0x5A5A, dtype=torch.int16, device="cuda")
    youth_filter.depth_filter_device(d_in, d_out, 8, 96)
    _memory_cap.mark()
    interior = lf.periodic_interior(lambda r: ft.filter_truth(r, 8, 96), block, FLT_HALO)
    for kind, phase in enumerate(phases):
        want = _filter_expected(block, H, phase, interior)
        assert not any(torch.equal(want, d_in[g]) for g in (0, 1, n - 2, n - 1))
        for f in np.nonzero(kinds == kind)[0]:
            _assert_equal(d_out[f], want, f"filter frame {f} of {n}")
        _memory_cap.mark()                              # the batch and an expected frame live
        del want
    _memory_cap.mark()


def test_filter_65535_frames_3x3(_memory_cap):
    """C: 65535 different 3 x 3 frames in one call; 65536 are refused and the
    output stays as it was."""
    n, W, H = lf.MAX_FRAMES, 3, 3
    frames = lf.counter_depth(n + 1, H, W)
    want = lf.unstack(ft.filter_truth(lf.stack_with_gaps(frames[:n], 2), 8, 96), n, H, 2)
    assert np.array_equal(want[n - 1], ft.filter_truth(frames[n - 1], 8, 96))
    assert len(np.unique(frames[:n].reshape(n, -1), axis=0)) > n // 2
    d_in = _cuda(frames)
    d_out = torch.full((n + 1, H, W), 0x5A5A, dtype=torch.int16, device="cuda")
    with pytest.raises(youth_icp.IcpError) as e:
        youth_filter.depth_filter_device(d_in, d_out, 8, 96)
    assert e.value.code == youth_icp.YOUTH_EINVAL
    torch.cuda.synchronize()
    assert (d_out == 0x5A5A).all()
    youth_filter.depth_filter_device(d_in[:n], d_out[:n], 8, 96)
    _assert_equal(d_out[:n], _cuda(want), "filter 65535 x 3x3")
    assert (d_out[n] == 0x5A5A).all()
    assert int((want != frames[:n]).sum()) > n


# ================================================================ viewer cloud ==

CLOUD_VALID = 200_000
CLOUD_K = youth_icp.Intrinsics(7000.25, 6990.5, 4090.75, 4101.5, 1000.0)


def _pose12(seed):
    """A camera -> world pose, row-major 3 x 4 fp32."""
    rng = np.random.default_rng(seed)
    w = rng.normal(size=3) * 0.4
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    return np.hstack([R, rng.normal(size=(3, 1))]).astype(np.float32)


def _check_cloud_frame(words, f, N, count, want):
    """Frame f of the guarded vertex words on the device: the list bit for bit,
    NAN_BITS behind it."""
    frame = words[f * N * 6:(f + 1) * N * 6]
    assert count == want.shape[0], (f, count, want.shape[0])
    want_w = _cuda(np.ascontiguousarray(want, np.float32).view(np.int32).reshape(-1))
    _assert_equal(frame[:count * 6], want_w, f"cloud frame {f}")
    assert int((frame[count * 6:] != NAN_BITS).sum()) == 0, f


@pytest.mark.parametrize("px", [8, 4])
@pytest.mark.parametrize("shape", lf.shapes(1) + [(8191, 8193)], ids=lf.shape_id)
def test_cloud_largest_frames(shape, px, monkeypatch, _memory_cap):
    """A: the device API at both tile widths, with and without colour, with and
    without a pose, on sparse frames; at 2^26 pixels k_cloud_scan's run length
    is 128 (8 px per thread) and 256 (4).  8191 x 8193 adds the scalar-load
    path and a partial last tile at 2^26 - 1 pixels."""
    monkeypatch.setenv("YOUTH_CLOUD_PX", str(px))
    W, H = shape
    N = W * H
    assert lf.admitted(W, H, 1)
    idx = lf.sparse_pixels(W, H, CLOUD_VALID, 17 + W)
    cnt = lf.sparse_counters(idx, W, H, 256 * px)
    assert cnt["corners"] and cnt["last_tile_valid"] >= 1
    assert cnt["R"] == (N + 256 * px * 256 - 1) // (256 * px * 256)
    if N >= lf.MAX_PIXELS - 1:
        assert cnt["R"] == (128 if px == 8 else 256)
    if shape == (8191, 8193):
        assert cnt["last_tile_partial"] and N % px
    depth, rgb = lf.sparse_depth(W, H, idx, 5), lf.sparse_rgb(W, H, idx, 5)
    assert int((depth > 0).sum()) == idx.size
    T = _pose12(W + H)
    K = CLOUD_K if W > 1 and H > 1 else None
    Kt = None if K is None else K.as_tuple()
    d_depth, d_rgb, d_T = _cuda(depth), _cuda(rgb), _cuda(T.reshape(1, 12))
    counts = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    with youth_viewer.CloudBuilder(W, H, max_frames=1) as cb:
        for colour in (True, False):
            for posed in (True, False):
                words = guarded_vertices(1, N)
                counts.fill_(-1)
                _ready()
                cb.build_device_posed(d_depth.data_ptr(), d_rgb.data_ptr() if colour else 0, 1, W, H,
                                      d_T.data_ptr() if posed else 0, words.data_ptr(),
                                      counts.data_ptr(), K=K)
                torch.cuda.synchronize()
                _memory_cap.mark()
                want = oracle.viewer_cloud(depth, rgb if colour else None, Kt,
                                           T_world=T if posed else None)
                assert want.shape[0] == idx.size
                _check_cloud_frame(words, 0, N, int(counts[0]), want)
                assert (words[N * 6:] == NAN_BITS).all()
                del words


def test_cloud_batch_past_4_gib_4x8192x8192(_memory_cap):
    """B: 4 sparse frames of 2^26 pixels: the vertex stride is N * 24 bytes
    whatever the counts, so frame 3's list starts at byte 4.5 * 2^30."""
    W, H, n = 8192, 8192, lf.smallest_batch_past_32_bits(24 * lf.MAX_PIXELS)
    N = W * H
    assert n == 4 and lf.last_frame_offset(n, 24 * N) >= 1 << 32
    frames = []
    for f in range(n):
        idx = lf.sparse_pixels(W, H, 50_000 + 1000 * f, 40 + f)
        frames.append((lf.sparse_depth(W, H, idx, 60 + f), idx))
    T = np.stack([_pose12(70 + f) for f in range(n)])
    d_depth = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
    for f in range(n):
        d_depth[f] = _cuda(frames[f][0])
    d_T = _cuda(T.reshape(n, 12))
    words = guarded_vertices(n, N)
    counts = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    _ready()
    with youth_viewer.CloudBuilder(W, H, max_frames=n) as cb:
        cb.build_device_posed(d_depth.data_ptr(), 0, n, W, H, d_T.data_ptr(), words.data_ptr(),
                              counts.data_ptr(), K=CLOUD_K)
        torch.cuda.synchronize()
        _memory_cap.mark()
    got = counts.cpu().numpy()
    for f in range(n):
        want = oracle.viewer_cloud(frames[f][0], None, CLOUD_K.as_tuple(), T_world=T[f])
        assert want.shape[0] == frames[f][1].size
        _check_cloud_frame(words, f, N, int(got[f]), want)
    assert (words[n * N * 6:] == NAN_BITS).all()


@pytest.mark.parametrize("px", [8, 4])
def test_cloud_65535_frames_1x1(px, monkeypatch, _memory_cap):
    """C: 65535 frames of one pixel, each with its own depth, colour and pose;
    65536 are refused (by create and by the build) and nothing is written."""
    monkeypatch.setenv("YOUTH_CLOUD_PX", str(px))
    n = lf.MAX_FRAMES
    depth = lf.counter_depth(n, 1, 1)
    rgb = (np.arange(n * 3, dtype=np.int64) * 29 % 256).astype(np.uint8).reshape(n, 1, 1, 3)
    T = np.tile(_pose12(9).reshape(1, 12), (n, 1))
    T[:, 3] += np.arange(n, dtype=np.float32) / 64
    K = youth_icp.Intrinsics(1.5, 2.5, 0.25, -0.5, 1000.0)
    d_depth, d_rgb, d_T = _cuda(depth), _cuda(rgb), _cuda(T)
    words = guarded_vertices(n, 1)
    counts = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(youth_icp.IcpError) as e:
        youth_viewer.CloudBuilder(1, 1, max_frames=n + 1)
    assert "1 <= frames <= 65535" in str(e.value)       # the frame count, not an allocation
    _ready()
    with youth_viewer.CloudBuilder(1, 1, max_frames=n) as cb:
        with pytest.raises(youth_icp.IcpError) as e:
            cb.build_device_posed(d_depth.data_ptr(), d_rgb.data_ptr(), n + 1, 1, 1, d_T.data_ptr(),
                                  words.data_ptr(), counts.data_ptr(), K=K)
        assert e.value.code == youth_icp.YOUTH_EINVAL
        torch.cuda.synchronize()
        assert (words == NAN_BITS).all() and (counts == -1).all()
        cb.build_device_posed(d_depth.data_ptr(), d_rgb.data_ptr(), n, 1, 1, d_T.data_ptr(),
                              words.data_ptr(), counts.data_ptr(), K=K)
        torch.cuda.synchronize()
    want_counts = (depth.reshape(n) > 0).astype(np.int32)
    assert 0 < want_counts.sum() < n
    want = np.full((n, 6), NAN_BITS, np.uint32)
    for f in np.nonzero(want_counts)[0]:
        v = oracle.viewer_cloud(depth[f], rgb[f], K.as_tuple(), T_world=T[f].reshape(3, 4))
        want[f] = v.view(np.uint32)[0]
    assert np.array_equal(counts[:n].cpu().numpy(), want_counts) and int(counts[n]) == -1
    got = words.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:n * 6].reshape(n, 6), want)
    assert (got[n * 6:] == NAN_BITS).all() and got.size == n * 6 + GUARD


# ============================================================== loop signature ==

def _signature_frame(W, H, seed):
    """Depth and intensity of W x H from vectors of a prime length laid over
    the frame (neighbouring rows differ; 2^26 fresh random numbers would cost
    more than the truth), with the holes of test_gpu_loop.py's frames: cells
    without depth and cells around the 4 cnt >= n threshold."""
    rng = np.random.default_rng(seed)
    P = 1_000_003
    dv = rng.integers(300, 32768, P).astype(np.int16)
    dv[rng.random(P) < 0.25] = 0
    dv[rng.random(P) < 0.05] = -7
    d = np.resize(dv, H * W).reshape(H, W)
    d[: H // 3, : W // 4] = 0
    keep = np.resize(rng.random(P) < 0.25, (H - H // 2) * (W - W // 2)).reshape(H - H // 2, W - W // 2)
    d[H // 2:, W // 2:] = np.where(keep, 32767, 0)
    y = np.resize(rng.integers(0, 256, P).astype(np.uint8), H * W).reshape(H, W)
    return d, y


def _run_signature(d, y, offset):
    n = 1 if d.ndim == 2 else d.shape[0]
    H, W = d.shape[-2:]
    td = torch.zeros(d.size + 16, dtype=torch.int16, device="cuda")
    ty = torch.zeros(y.size + 32, dtype=torch.uint8, device="cuda")
    od, oy = offset // 2, offset
    td[od:od + d.size] = _cuda(d.reshape(-1))
    ty[oy:oy + y.size] = _cuda(y.reshape(-1))
    sig = torch.full((n + 1, 300), 0xDEAD, dtype=torch.int32, device="cuda")
    youth_loop.signature_device(td.data_ptr() + 2 * od, ty.data_ptr() + oy, n, W, H, sig.data_ptr())
    torch.cuda.synchronize()
    s = sig.cpu().numpy().view(np.uint32)
    assert (s[n] == 0xDEAD).all()
    return s[:n]


@pytest.mark.parametrize("shape", lf.BIG + [(16384, 15), (20, 16384)], ids=lf.shape_id)
def test_signature_largest_frames(shape, _memory_cap):
    """A: on 16-byte aligned planes (where W % 16 == 0: the vector loads) and
    on planes 2 bytes off (element loads)."""
    W, H = shape
    assert lf.admitted(W, H, 20, 15)
    d, y = _signature_frame(W, H, W + 3 * H)
    want = loop_truth.signature(d, y)
    valid = want >> 31
    assert valid.any() and not valid.all()
    for offset in (0, 2):
        got = _run_signature(d, y, offset)
        _memory_cap.mark()
        assert np.array_equal(got[0], want), (offset, np.argwhere(got[0] != want)[:5])


def test_signature_65535_frames_20x15(_memory_cap):
    """C: 65535 different frames of 20 x 15, where a pixel is a cell; 65536 are
    refused and the records stay as they were."""
    n = lf.MAX_FRAMES
    d = lf.counter_depth(n + 1, 15, 20)
    y = (np.arange((n + 1) * 300, dtype=np.int64) * 13 % 256).astype(np.uint8).reshape(n + 1, 15, 20)
    want = lf.signature_20x15(d[:n], y[:n])
    for f in (0, 1, n // 2, n - 2, n - 1):
        assert np.array_equal(want[f], loop_truth.signature(d[f], y[f]))
    got = _run_signature(d[:n], y[:n], 0)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    td, ty = _cuda(d), _cuda(y)
    sig = torch.full((n + 1, 300), 0xDEAD, dtype=torch.int32, device="cuda")
    with pytest.raises(youth_icp.IcpError) as e:
        youth_loop.signature_device(td.data_ptr(), ty.data_ptr(), n + 1, 20, 15, sig.data_ptr())
    assert e.value.code == youth_icp.YOUTH_EINVAL
    torch.cuda.synchronize()
    assert (sig == 0xDEAD).all()


# =================================================================== rectifier ==

BARREL = (-0.12, 0.03, 0.001, -0.0007, 0.004)
NO_DISTORTION = (0.0, 0.0, 0.0, 0.0, 0.0)


def _strip_distortion(W, H):
    """BARREL without the tangential term that would push a 2-pixel side's
    source positions off the frame."""
    k1, k2, p1, p2, k3 = BARREL
    return (k1, k2, p1 if H > 2 else 0.0, p2 if W > 2 else 0.0, k3)


def _barrel_camera(W, H):
    """A camera whose field of view makes BARREL bite: focal length 0.7 of the
    longer side, the centre off the middle by a fraction of a pixel."""
    f = 0.7 * max(W, H)
    return youth_icp.Intrinsics(f, f * 1.01, W / 2 - 0.37, H / 2 - 0.21, 1000.0)


def _exact_camera(W, H):
    """fx a power of two and an integral centre: (u - cx) / fx * fx + cx is u
    in fp32, so without distortion every pixel maps onto itself."""
    return youth_icp.Intrinsics(8192.0, 8192.0, float(W // 2), float(H // 2), 1000.0)


def _rect_planes(W, H, n, seed):
    rng = np.random.default_rng(seed)
    d = (1200 + rng.integers(-40, 41, (n, H, W))).astype(np.int16)
    d[rng.random((n, H, W)) < 0.1] = 0
    d[rng.random((n, H, W)) < 0.02] = -5
    return d, rng.integers(0, 256, (n, H, W, 3)).astype(np.uint8), \
        rng.integers(0, 256, (n, H, W, 1)).astype(np.uint8)


@pytest.mark.parametrize("use_map", ["0", "1"], ids=["recompute", "map"])
@pytest.mark.parametrize("shape", [(16384, 2), (2, 16384), (16384, 64)], ids=lf.shape_id)
def test_rectify_strips_in_full(shape, use_map, monkeypatch, _memory_cap):
    """A: the distorted apply, depth and colour of 3 channels and of 1, and the
    map words, on the strips; at 16384 x 2 and 2 x 16384 the tap clamp
    min(V >> 5, H - 2) and min(U >> 5, W - 2) is at 0."""
    monkeypatch.setenv("YOUTH_RECTIFY_MAP", use_map)
    W, H = shape
    assert lf.admitted(W, H, 2)
    K, D = _barrel_camera(W, H), _strip_distortion(W, H)
    d, c3, c1 = _rect_planes(W, H, 2, W + H)
    parts = rectify_truth.map_parts(W, H, K, D)
    assert W * H // 2 < int(parts[0].sum()) <= W * H
    want_d, want_c3 = rectify_truth.rectify(d, c3, W, H, K, D)
    _, want_c1 = rectify_truth.rectify(None, c1, W, H, K, D)
    with youth_rectify.Rectifier(W, H, K, D) as r:
        assert r.covered == int(parts[0].sum())
        assert np.array_equal(r.map(), rectify_truth.map_words(W, H, K, D))
        got_d, got_c3 = r.device_frames(_cuda(d), None, _cuda(c3), None)
        _, got_c1 = r.device_frames(None, None, _cuda(c1), None)
        torch.cuda.synchronize()
        _memory_cap.mark()
    assert np.array_equal(got_d.cpu().numpy(), want_d)
    assert np.array_equal(got_c3.cpu().numpy(), want_c3)
    assert np.array_equal(got_c1.cpu().numpy(), want_c1)
    assert int((want_d != d).sum()) > W * H // 4


def _random_planes_on_device(W, H, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    d = torch.randint(-20, 9000, (1, H, W), generator=g, device="cuda", dtype=torch.int16)
    c3 = torch.randint(0, 256, (1, H, W, 3), generator=g, device="cuda", dtype=torch.uint8)
    return d, c3


@pytest.mark.parametrize("use_map", ["0", "1"], ids=["recompute", "map"])
@pytest.mark.parametrize("shape", lf.BIG, ids=lf.shape_id)
def test_rectify_largest_frames_without_distortion(shape, use_map, monkeypatch, _memory_cap):
    """A: under the no-distortion camera the output is the input, in the form
    that recomputes the map words and in the one that reads them."""
    monkeypatch.setenv("YOUTH_RECTIFY_MAP", use_map)
    W, H = shape
    K = _exact_camera(W, H)
    assert lf.admitted(W, H, 2) and lf.identity_map_holds(W, H, K.as_tuple())
    d, c3 = _random_planes_on_device(W, H, W)
    c1 = c3[..., :1].contiguous()
    with youth_rectify.Rectifier(W, H, K, NO_DISTORTION) as r:
        assert r.covered == W * H
        od = torch.full_like(d, 0x5A5A)
        oc = torch.full_like(c3, 0xA5)
        r.device_frames(d, od, c3, oc)
        o1 = torch.full_like(c1, 0xA5)
        r.device_frames(None, None, c1, o1)
        torch.cuda.synchronize()
        _memory_cap.mark()
    _assert_equal(od, d, "depth")
    _assert_equal(oc, c3, "colour")
    _assert_equal(o1, c1, "one channel")


def test_rectify_map_words_8192x8192(_memory_cap):
    """A: the map as data at 2^26 pixels under the barrel camera, every word;
    the output camera is wider than the sensor's, so the frame's rim is not
    covered."""
    W, H = 8192, 8192
    K = _barrel_camera(W, H)
    Ko = youth_icp.Intrinsics(0.8 * K.fx, 0.8 * K.fy, K.cx, K.cy, K.depth_scale)
    with youth_rectify.Rectifier(W, H, K, BARREL, Ko) as r:
        m = r.map_device()
        torch.cuda.synchronize()
        _memory_cap.mark()
        covered = r.covered
    want = rectify_truth.map_words(W, H, K, BARREL, Ko)
    assert 0 < covered < W * H and covered == int((want[..., 0] >> 31).sum())
    _assert_equal(m, _cuda(want.view(np.int32)), "map words")


def test_rectify_batch_past_4_gib_23x8192x8192(_memory_cap):
    """B: 23 colour-only frames of 2^26 pixels, 3 bytes a pixel: frame 22
    starts at byte 4.125 * 2^30.  Without distortion the output is the input,
    compared whole on the device."""
    W, H, n = 8192, 8192, lf.smallest_batch_past_32_bits(3 * lf.MAX_PIXELS)
    assert n == 23 and lf.last_frame_offset(n, 3 * W * H) >= 1 << 32
    K = _exact_camera(W, H)
    assert lf.identity_map_holds(W, H, K.as_tuple())
    kinds = lf.batch_kinds(n)
    c_in = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
    for kind in range(4):
        c = _random_planes_on_device(W, H, 90 + kind)[1][0]
        for f in np.nonzero(kinds == kind)[0]:
            c_in[f] = c
        del c
    assert not torch.equal(c_in[0], c_in[1]) and not torch.equal(c_in[n - 2], c_in[n - 1])
    c_out = torch.full_like(c_in, 0xA5)
    with youth_rectify.Rectifier(W, H, K, NO_DISTORTION) as r:
        r.device_frames(None, None, c_in, c_out)
        torch.cuda.synchronize()
        _memory_cap.mark()
    _memory_cap.mark()
    for f in range(n):
        _assert_equal(c_out[f], c_in[f], f"rectify frame {f} of {n}")


def test_rectify_65535_frames_2x2(_memory_cap):
    """C: 65535 different 2 x 2 frames, depth and colour, under a camera that
    puts fractional weights on every covered pixel; 65536 are refused."""
    n, W, H = lf.MAX_FRAMES, 2, 2
    K = youth_icp.Intrinsics(1.0, 1.25, 0.45, 0.4, 1000.0)
    Ko, D = youth_icp.Intrinsics(2.0, 2.5, 0.1, 0.2, 1000.0), (-0.2, 0.02, 0.01, -0.01, 0.0)
    parts = rectify_truth.map_parts(W, H, K, D, Ko)
    assert parts[0].all() and (parts[3] % 32 != 0).all() and (parts[4] % 32 != 0).all()
    d = lf.counter_depth(n + 1, H, W)
    d = np.where(d > 0, 1500 + d % 16, d).astype(np.int16)      # taps inside each other's gate
    c3 = (np.arange((n + 1) * 12, dtype=np.int64) * 37 % 256).astype(np.uint8).reshape(n + 1, H, W, 3)
    wide = lf.tile_parts(parts, n)
    want_d = lf.from_side_by_side(rectify_truth.rectify_depth(lf.side_by_side(d[:n]), wide), n)
    want_c = lf.from_side_by_side(rectify_truth.rectify_color(lf.side_by_side(c3[:n]), wide), n)
    for f in (0, n - 1):
        a, b = rectify_truth.rectify(d[f], c3[f], W, H, K, D, Ko)
        assert np.array_equal(a, want_d[f]) and np.array_equal(b, want_c[f])
    td, tc = _cuda(d), _cuda(c3)
    od, oc = torch.full_like(td, 0x5A5A), torch.full_like(tc, 0xA5)
    with youth_rectify.Rectifier(W, H, K, D, Ko) as r:
        with pytest.raises(youth_icp.IcpError) as e:
            r.device_frames(td, od, tc, oc)
        assert e.value.code == youth_icp.YOUTH_EINVAL
        torch.cuda.synchronize()
        assert (od == 0x5A5A).all() and (oc == 0xA5).all()
        r.device_frames(td[:n], od[:n], tc[:n], oc[:n])
        torch.cuda.synchronize()
    assert np.array_equal(od[:n].cpu().numpy(), want_d)
    assert np.array_equal(oc[:n].cpu().numpy(), want_c)
    assert (od[n] == 0x5A5A).all() and (oc[n] == 0xA5).all()
    assert int((want_d != d[:n]).sum()) > n


# =================================================================== voxel map ==

MAP_VALID = 150_000


def _same_records(got, want, what=""):
    assert got.dtype == want.dtype == youth_map.VOXEL_DTYPE
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), what


def _map_clean(m, removed):
    """Nothing dropped, missing, underflowed or stale; `removed` points out."""
    st, rs = m.stats(), m.remove_stats()
    assert st["dropped"] == 0 and st["out_of_range"] == 0, st
    assert rs["missing"] == rs["underflow"] == rs["stale"] == 0 and rs["removed"] == removed, rs
    assert rs["live"] + rs["vacant"] == st["occupied"]
    return st, rs


@pytest.mark.parametrize("lds", ["1", "0"], ids=["lds", "direct"])
@pytest.mark.parametrize("shape", lf.shapes(1), ids=lf.shape_id)
def test_map_largest_frames(shape, lds, monkeypatch, _memory_cap):
    """A: one sparse coloured frame in, the same frame out again (the extract
    is empty and remove_stats exact), in once more and moved to a second pose;
    with the LDS table and without."""
    monkeypatch.setenv("YOUTH_MAP_LDS", lds)
    W, H = shape
    N, vpm = W * H, 100.0
    assert lf.admitted(W, H, 1)
    idx = lf.sparse_pixels(W, H, MAP_VALID, 23 + W)
    cnt = lf.sparse_counters(idx, W, H, 2048)
    assert cnt["corners"] and cnt["last_tile_valid"] >= 1
    depth, rgb = lf.sparse_depth(W, H, idx, 9), lf.sparse_rgb(W, H, idx, 9)
    valid = idx.size
    K = CLOUD_K if W > 1 and H > 1 else None
    T = np.stack([_pose12(W), _pose12(H + 1)])
    want = [map_truth.restate(*map_truth.frame_points(depth, rgb, K, T[k]), vpm) for k in range(2)]
    assert want[0][1] == want[1][1] == 0 and want[0][0].shape[0] > valid // 2
    assert want[0][0].tobytes() != want[1][0].tobytes()
    d_depth, d_rgb, d_T = _cuda(depth), _cuda(rgb), _cuda(T.reshape(2, 12))
    args = (d_depth.data_ptr(), d_rgb.data_ptr(), 1, W, H)
    _ready()
    with youth_map.VoxelMap(vpm, slots=1 << 20) as m:
        m.integrate_device(*args, d_T.data_ptr(), K)
        _same_records(m.extract(), want[0][0], "integrate")
        st = m.stats()
        assert st["integrated"] == valid and (st["direct"] == valid) == (lds == "0")
        _memory_cap.mark()
        m.remove_device(*args, d_T.data_ptr(), K)
        assert m.extract().shape == (0,)
        st, rs = _map_clean(m, removed=valid)
        assert rs["live"] == 0 and rs["vacant"] == st["occupied"] == want[0][0].shape[0]
        m.integrate_device(*args, d_T.data_ptr(), K)
        _same_records(m.extract(), want[0][0], "integrate again")
        m.move_device(*args, d_T.data_ptr(), d_T.data_ptr() + 48, K)
        _same_records(m.extract(), want[1][0], "move")
        _map_clean(m, removed=2 * valid)
        assert m.stats()["integrated"] == 3 * valid


@pytest.mark.parametrize("colour", [False, True], ids=["33_colourless", "23_coloured"])
def test_map_batch_past_4_gib_8192x8192(colour, _memory_cap):
    """B: 33 colourless frames (2 bytes a pixel: frame 32's depth starts at byte
    2^32) and 23 coloured ones (frame 22's colour starts at byte 4.125 * 2^30),
    sparse; frames of a kind share their pose."""
    W, H = 8192, 8192
    N, vpm = W * H, 100.0
    n = lf.smallest_batch_past_32_bits((3 if colour else 2) * N)
    assert n == (23 if colour else 33) and lf.last_frame_offset(n, (3 if colour else 2) * N) >= 1 << 32
    kinds = lf.batch_kinds(n)
    frames, pts = [], []
    for k in range(4):
        idx = lf.sparse_pixels(W, H, 6000 + 500 * k, 300 + k)
        d = lf.sparse_depth(W, H, idx, 310 + k)
        c = lf.sparse_rgb(W, H, idx, 320 + k) if colour else None
        T = _pose12(330 + k)
        frames.append((d, c, T))
        pts.append(map_truth.frame_points(d, c, CLOUD_K, T))
    want, oor = map_truth.restate(np.concatenate([pts[k][0] for k in kinds]),
                                  np.concatenate([pts[k][1] for k in kinds]), vpm)
    valid = int(sum(pts[k][0].shape[0] for k in kinds))
    assert oor == 0 and int(want["count"].max()) >= n - 3
    d_depth = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
    d_rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda") if colour else None
    for k in range(4):
        dk = _cuda(frames[k][0])
        ck = _cuda(frames[k][1]) if colour else None
        for f in np.nonzero(kinds == k)[0]:
            d_depth[f] = dk
            if colour:
                d_rgb[f] = ck
        del dk, ck
    d_T = _cuda(np.stack([frames[k][2] for k in kinds]).reshape(n, 12))
    args = (d_depth.data_ptr(), d_rgb.data_ptr() if colour else 0, n, W, H, d_T.data_ptr(), CLOUD_K)
    _ready()
    with youth_map.VoxelMap(vpm, slots=1 << 18) as m:
        m.integrate_device(*args)
        _same_records(m.extract(), want, "integrate")
        assert m.stats()["integrated"] == valid
        _memory_cap.mark()
        m.remove_device(*args)
        assert m.extract().shape == (0,)
        _map_clean(m, removed=valid)


@pytest.mark.parametrize("lds", ["1", "0"], ids=["lds", "direct"])
def test_map_65535_frames_1x1(lds, monkeypatch, _memory_cap):
    """C: 65535 frames of one pixel in one integrate, each with its own depth,
    colour and pose; 65536 are refused and the map stays as it was."""
    monkeypatch.setenv("YOUTH_MAP_LDS", lds)
    n, vpm = lf.MAX_FRAMES, 50.0
    depth = lf.counter_depth(n + 1, 1, 1)
    rgb = (np.arange((n + 1) * 3, dtype=np.int64) * 29 % 256).astype(np.uint8).reshape(n + 1, 1, 1, 3)
    T = np.tile(_pose12(19).reshape(1, 12), (n + 1, 1))
    T[:, 3] += np.arange(n + 1, dtype=np.float32) / 128
    T[:, 7] -= (np.arange(n + 1) % 97).astype(np.float32) / 16
    K = youth_icp.Intrinsics(1.5, 2.5, 0.25, -0.5, 1000.0)
    live = np.nonzero(depth[:n].reshape(n) > 0)[0]
    P = np.concatenate([-oracle.viewer_cloud(depth[f], None, K.as_tuple(), T_world=T[f].reshape(3, 4))[:, :3]
                        for f in live])
    want, oor = map_truth.restate(P, rgb[live].reshape(-1, 3), vpm)
    assert oor == 0 and 0 < live.size < n and want.shape[0] > n // 8
    d_depth, d_rgb, d_T = _cuda(depth), _cuda(rgb), _cuda(T)
    _ready()
    with youth_map.VoxelMap(vpm, slots=1 << 18) as m:
        m.integrate_device(d_depth.data_ptr(), d_rgb.data_ptr(), n, 1, 1, d_T.data_ptr(), K)
        _same_records(m.extract(), want)
        st = m.stats()
        assert st["integrated"] == live.size and st["dropped"] == 0
        with pytest.raises(youth_icp.IcpError) as e:
            m.integrate_device(d_depth.data_ptr(), d_rgb.data_ptr(), n + 1, 1, 1, d_T.data_ptr(), K)
        assert e.value.code == youth_icp.YOUTH_EINVAL
        _same_records(m.extract(), want)
        assert m.stats() == st


def _render_views(m, Vs, W, H, K, max_splat=0, rgb=True):
    """render_device of the views Vs ([n][3][4] fp32) -> (depth [n][H][W],
    rgb [n][H][W][3] or None) on the device, pre-filled with 0x5A."""
    n = len(Vs)
    d_V = _cuda(np.asarray(Vs, np.float32).reshape(n, 12))
    d_d = torch.full((n, H, W), 0x5A5A, dtype=torch.int16, device="cuda")
    d_c = torch.full((n, H, W, 3), 0x5A, dtype=torch.uint8, device="cuda") if rgb else None
    _ready()
    m.render_device(d_V.data_ptr(), d_d.data_ptr(), d_c.data_ptr() if rgb else 0, n, W, H, K,
                    max_splat=max_splat)
    m.sync()
    return d_d, d_c


@pytest.mark.parametrize("lds", ["1", "0"], ids=["lds", "direct"])
def test_map_boundary_cells(lds, monkeypatch, _memory_cap):
    """D: 2^20 voxels per metre, so the 21-bit cells end at -1 m and 1 m.  One
    integrate of hand-made points (a 1 x 1 frame each, the pose all
    translation, which the fp32 chain reproduces exactly: asserted with
    frame_points): the eight corner cells -2^20 / 2^20 - 1, an fp32 step inside
    the faces, out of range on exactly one axis (1.0 and nextafter(-1, -2)),
    ordinary ones.  Records, out_of_range and integrated exact; removed again;
    then the corner voxels rendered from the front and from behind on both
    splat paths."""
    monkeypatch.setenv("YOUTH_MAP_LDS", lds)
    vpm = lf.BOUNDARY_VPM
    P, cls = lf.boundary_points()
    depth, rgb, T = lf.point_frames(P)
    n = P.shape[0]
    fp = [map_truth.frame_points(depth[f], rgb[f], None, T[f].reshape(3, 4)) for f in range(n)]
    got_P = np.concatenate([p for p, _ in fp])
    assert np.array_equal(got_P.view(np.uint32), P.view(np.uint32))
    ok, cell, q = map_truth.keys_of(P, vpm)
    count = dict(zip(*np.unique(cls, return_counts=True)))
    assert count == {"corner": 8, "near": 3, "out": 6, "ordinary": 8}
    assert ok[cls != "out"].all() and not ok[cls == "out"].any()
    corner = cell[:8]
    assert set(np.unique(corner)) == {lf.CELL_MIN, lf.CELL_MAX} and len({tuple(c) for c in corner}) == 8
    assert (q[:8][corner == lf.CELL_MAX] == 240).all() and (q[:8][corner == lf.CELL_MIN] == 0).all()
    want, oor = map_truth.restate(P, np.concatenate([c for _, c in fp]), vpm)
    assert oor == 6 and want.shape[0] == 17 and int(want["count"].sum()) == n - 6
    d_depth, d_rgb, d_T = _cuda(depth), _cuda(rgb), _cuda(T)
    args = (d_depth.data_ptr(), d_rgb.data_ptr(), n, 1, 1, d_T.data_ptr())
    Kv = youth_icp.Intrinsics(16.0, 16.0, 32.0, 32.0, 1000.0)
    Vs = [render_truth.view_from_pose(Tw) for Tw in (np.eye(4), np.diag([-1.0, 1.0, -1.0, 1.0]))]
    renders = {}
    for queue in ("1", "0"):
        monkeypatch.setenv("YOUTH_MAP_RENDER_QUEUE", queue)
        _ready()
        with youth_map.VoxelMap(vpm, slots=64) as m:
            m.integrate_device(*args)
            _same_records(m.extract(), want)
            st = m.stats()
            assert st["out_of_range"] == 6 and st["integrated"] == n - 6 and st["dropped"] == 0
            m.remove_device(*args)
            assert m.extract().shape == (0,)
            rs = m.remove_stats()
            assert rs["removed"] == n - 6 and rs["missing"] == rs["underflow"] == rs["stale"] == 0
            assert rs["live"] == 0 and rs["vacant"] == 17
            m.integrate_device(*args)
            _same_records(m.extract(), want)
            d_d, d_c = _render_views(m, Vs, 64, 64, Kv)
            renders[queue] = (d_d.cpu().numpy(), d_c.cpu().numpy())
    for k, V in enumerate(Vs):
        corners = want[(np.abs(want["ix"] + 0.5) > (1 << 20) - 1) & (np.abs(want["iy"] + 0.5) > (1 << 20) - 1)
                       & (np.abs(want["iz"] + 0.5) > (1 << 20) - 1)]
        assert corners.shape[0] == 8
        assert render_truth.project(corners, vpm, V, Kv, 64, 64)[0].size == 4     # the four in front
        wd, wc = render_truth.render(want, vpm, V, Kv, 64, 64)
        assert all(wd[y, x] > 0 for y in (16, 48) for x in (16, 48))
        for queue in ("1", "0"):
            assert np.array_equal(renders[queue][0][k], wd) and np.array_equal(renders[queue][1][k], wc)


def test_map_smallest_table(_memory_cap):
    """D: slots = 1 gives 64.  64 different voxels fill it (the probe bound of
    128 reaches every slot), a 65th finds no room and is dropped and counted;
    everything out, in again, out again; compaction of the vacated table
    leaves no voxel and room for the 65th."""
    d64, c64, Kt = lf.distinct_voxel_frame(64)
    K = youth_icp.Intrinsics(*Kt)
    T65 = np.array([[1, 0, 0, 500.0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float64)
    want64, _ = map_truth.restate(*map_truth.frame_points(d64, c64, K), 1.0)
    want65, _ = map_truth.restate(*map_truth.frame_points(d64[:, :1], c64[:, :1], K, T65), 1.0)
    assert want64.shape[0] == 64 and (want64["count"] == 1).all() and want65.shape[0] == 1
    assert not np.isin(want65["ix"], want64["ix"]).any()
    with youth_map.VoxelMap(1.0, slots=1) as m:
        assert m.stats()["capacity"] == 64
        m.integrate(d64, c64, K)
        _same_records(m.extract(), want64, "64 voxels")
        st = m.stats()
        assert st["occupied"] == 64 == m.voxels() and st["dropped"] == 0 and st["integrated"] == 64
        m.integrate(d64[:, :1], c64[:, :1], K, T65)            # returns: probing is bounded
        got, st = m.extract(), m.stats()
        _same_records(got, want64, "the 65th changes nothing")
        # test_full_table_drops_and_counts' invariants: a subset of the truth,
        # every valid point either in a record or counted as dropped
        assert st["dropped"] == 1 and st["dropped"] + int(got["count"].sum()) == 65
        assert st["integrated"] == int(got["count"].sum()) == 64 and st["occupied"] == 64
        m.remove(d64, c64, K)
        assert m.extract().shape == (0,)
        rs = m.remove_stats()
        assert rs["removed"] == 64 and rs["live"] == 0 and rs["vacant"] == 64
        assert rs["missing"] == rs["underflow"] == rs["stale"] == 0
        m.integrate(d64, c64, K)                                # every voxel finds its kept slot
        _same_records(m.extract(), want64, "in again")
        assert m.stats()["dropped"] == 1
        m.remove(d64, c64, K)
        m.compact()
        assert m.voxels() == 0 and m.extract().shape == (0,)
        rs = m.remove_stats()
        assert rs["live"] == rs["vacant"] == rs["stale"] == 0
        m.integrate(d64[:, :1], c64[:, :1], K, T65)
        _same_records(m.extract(), want65, "the 65th after compaction")
        assert m.stats()["dropped"] == 1


# ==================================================================== renderer ==

RENDER_VPM = 100.0


def _render_scene():
    """About 2 * 10^4 voxels 1 to 4 m in front of the origin, within +-45
    degrees across and +-27 up and down."""
    rng = np.random.default_rng(31)
    depth = rng.integers(1000, 4000, (100, 200)).astype(np.int16)
    rgb = rng.integers(0, 256, (100, 200, 3)).astype(np.uint8)
    return depth, rgb, youth_icp.Intrinsics(100.0, 100.0, 100.0, 50.0, 1000.0)


def _render_camera(W, H):
    """The scene's +-1 by +-0.5 of x / z and y / z spread over the whole view,
    some of it past the rim; the focal length is at least 2000, so that near
    voxels have footprints of 16 x 16 in the narrow views too."""
    return youth_icp.Intrinsics(max(0.55 * W, 2000.0), 1.1 * H, W / 2 + 0.25, H / 2 - 0.25, 1000.0)


def _view(seed, shift=0.0):
    """A view a few degrees and centimetres off the scene's camera."""
    rng = np.random.default_rng(seed)
    T = np.vstack([_pose12(seed), [0, 0, 0, 1]]).astype(np.float64)
    T[:3, :3] = np.eye(3) + 0.1 * (T[:3, :3] - np.eye(3))
    u, _, vt = np.linalg.svd(T[:3, :3])
    T[:3, :3] = u @ vt
    T[:3, 3] = rng.normal(size=3) * 0.05 + shift
    return render_truth.view_from_pose(T)


def _scene_map(m):
    depth, rgb, K = _render_scene()
    m.integrate(depth, rgb, K)
    rec = m.extract()
    assert 10_000 < rec.shape[0] and m.stats()["dropped"] == 0
    return rec


@pytest.mark.parametrize("max_splat", [16, 1])
@pytest.mark.parametrize("shape", lf.shapes(1), ids=lf.shape_id)
def test_render_largest_views(shape, max_splat, monkeypatch, _memory_cap):
    """A: a map of 2 * 10^4 voxels into one view of each shape, footprints of
    16 x 16 and of one pixel, on both splat paths: the truth's bytes twice."""
    W, H = shape
    assert lf.admitted(W, H, 1)
    K, V = _render_camera(W, H), _view(W + max_splat)
    want = None
    for queue in ("1", "0"):
        monkeypatch.setenv("YOUTH_MAP_RENDER_QUEUE", queue)
        with youth_map.VoxelMap(RENDER_VPM, slots=1 << 16) as m:
            rec = _scene_map(m)
            if want is None:
                u0, v0, s, _ = render_truth.project(rec, RENDER_VPM, V, K, W, H, max_splat)
                assert u0.size > 200 and int(s.max()) == max_splat
                over = (u0 < 0) | (v0 < 0) | (u0 + s > W) | (v0 + s > H)
                # footprints past the rim and, where the view has room for one, whole ones
                assert over.any() and (min(W, H) < max_splat or not over.all())
                wd, wc = render_truth.render(rec, RENDER_VPM, V, K, W, H, max_splat)
                want = _cuda(wd[None]), _cuda(wc[None])
            d_d, d_c = _render_views(m, [V], W, H, K, max_splat)
            _memory_cap.mark()
            _assert_equal(d_d, want[0], f"depth, queue {queue}")
            _assert_equal(d_c, want[1], f"colour, queue {queue}")
            del d_d, d_c


@pytest.mark.parametrize("queue", ["1", "0"], ids=["queue", "walk"])
def test_render_batch_past_4_gib_9x8192x8192(queue, monkeypatch, _memory_cap):
    """B: 9 views of 2^26 pixels: 8 bytes a z-buffer pixel, view 8's z-buffer
    starts at byte 2^32."""
    monkeypatch.setenv("YOUTH_MAP_RENDER_QUEUE", queue)
    W, H, n = 8192, 8192, lf.smallest_batch_past_32_bits(8 * lf.MAX_PIXELS)
    assert n == 9 and lf.last_frame_offset(n, 8 * W * H) >= 1 << 32
    kinds = lf.batch_kinds(n)
    K = _render_camera(W, H)
    Vk = [_view(50 + k, shift=0.1 * k) for k in range(4)]
    with youth_map.VoxelMap(RENDER_VPM, slots=1 << 16) as m:
        rec = _scene_map(m)
        d_d, d_c = _render_views(m, [Vk[k] for k in kinds], W, H, K, 4)
        _memory_cap.mark()
    for k in range(4):
        wd, wc = render_truth.render(rec, RENDER_VPM, Vk[k], K, W, H, 4)
        assert (wd > 0).sum() > 50_000
        td, tc = _cuda(wd), _cuda(wc)
        assert not any(torch.equal(td, d_d[f]) for f in np.nonzero(kinds != k)[0][:3])
        for f in np.nonzero(kinds == k)[0]:
            _assert_equal(d_d[f], td, f"depth of view {f}")
            _assert_equal(d_c[f], tc, f"colour of view {f}")
        del td, tc


@pytest.mark.parametrize("queue", ["1", "0"], ids=["queue", "walk"])
def test_render_65535_views_1x1(queue, monkeypatch, _memory_cap):
    """C: 65535 views of one pixel, every one from another place; 65536 are
    refused and the outputs stay as they were."""
    monkeypatch.setenv("YOUTH_MAP_RENDER_QUEUE", queue)
    n, vpm = lf.MAX_FRAMES, 20.0
    K = youth_icp.Intrinsics(2.0, 2.0, 0.5, 0.5, 1000.0)
    depth = np.array([[1500, 2500, 0], [3500, 800, 2000]], np.int16)
    rgb = (np.arange(18) * 13 % 256).astype(np.uint8).reshape(2, 3, 3)
    V = np.tile(np.eye(4, dtype=np.float32)[:3].reshape(1, 12), (n, 1))
    f = np.arange(n)
    V[:, 3] = ((f % 41) - 20).astype(np.float32) / 16           # world -> camera shifts
    V[:, 7] = ((f // 41 % 41) - 20).astype(np.float32) / 16
    V[:, 11] = (f // 1681).astype(np.float32) / 8 - 1.0
    with youth_map.VoxelMap(vpm, slots=64) as m:
        m.integrate(depth, rgb, youth_icp.Intrinsics(2.0, 2.0, 1.0, 0.5, 1000.0))
        rec = m.extract()
        assert rec.shape[0] == 5
        d_V = _cuda(V)
        d_d = torch.full((n + 1,), 0x5A5A, dtype=torch.int16, device="cuda")
        d_c = torch.full((n + 1, 3), 0x5A, dtype=torch.uint8, device="cuda")
        _ready()
        with pytest.raises(youth_icp.IcpError) as e:
            m.render_device(d_V.data_ptr(), d_d.data_ptr(), d_c.data_ptr(), n + 1, 1, 1, K)
        assert e.value.code == youth_icp.YOUTH_EINVAL
        m.sync()
        assert (d_d == 0x5A5A).all() and (d_c == 0x5A).all()
        m.render_device(d_V.data_ptr(), d_d.data_ptr(), d_c.data_ptr(), n, 1, 1, K)
        m.sync()
    wd, wc = np.zeros(n, np.int16), np.zeros((n, 3), np.uint8)
    for k in range(n):
        a, b = render_truth.render(rec, vpm, V[k], K, 1, 1)
        wd[k], wc[k] = a[0, 0], b[0, 0]
    assert n // 20 < int((wd > 0).sum()) < n and len(np.unique(wd)) > 20
    assert np.array_equal(d_d[:n].cpu().numpy(), wd) and np.array_equal(d_c[:n].cpu().numpy(), wc)
    assert int(d_d[n]) == 0x5A5A and (d_c[n] == 0x5A).all()


def test_render_queue_saturated(monkeypatch, _memory_cap):
    """D: a table of 1024 slots, one tile of k_map_render_splat, filled to the
    brim by a cluster of 1-mm voxels so near the view camera that every one
    survives the culls with an unclipped 16 x 16 footprint: the queue holds
    1024 entries and its prefix ends at 1023 * 256 pixels.  Each splat path
    fills a map of its own, which keeps its own 1024 of the cluster's voxels,
    so each is held to the truth of its own records."""
    depth, rgb = lf.queue_frame()
    Kin, Kv = youth_icp.Intrinsics(*lf.QUEUE_K_IN), youth_icp.Intrinsics(*lf.QUEUE_K_VIEW)
    W, H = lf.QUEUE_VIEW
    V = np.eye(4, dtype=np.float32)[:3]
    full, _ = map_truth.restate(*map_truth.frame_points(depth, rgb, Kin), lf.QUEUE_VPM)
    assert full.shape[0] > 10 * lf.QUEUE_SLOTS
    for queue in ("1", "0"):
        monkeypatch.setenv("YOUTH_MAP_RENDER_QUEUE", queue)
        with youth_map.VoxelMap(lf.QUEUE_VPM, slots=lf.QUEUE_SLOTS) as m:
            m.integrate(depth, rgb, Kin)
            rec, st = m.extract(), m.stats()
            assert st["capacity"] == lf.QUEUE_SLOTS == st["occupied"] == rec.shape[0]
            assert st["dropped"] + int(rec["count"].sum()) == int((depth > 0).sum())
            u0, v0, s, _ = render_truth.project(rec, lf.QUEUE_VPM, V, Kv, W, H)
            assert lf.queue_counters(u0, v0, s, rec.shape[0], W, H) == \
                {"records": 1024, "survivors": 1024, "whole_16x16": 1024}
            d_d, d_c = _render_views(m, [V], W, H, Kv)
            wd, wc = render_truth.render(rec, lf.QUEUE_VPM, V, Kv, W, H)
            assert np.array_equal(d_d[0].cpu().numpy(), wd), queue
            assert np.array_equal(d_c[0].cpu().numpy(), wc), queue
            # a record of the table is one of the frame's voxels, no sum above the truth's
            at = np.searchsorted(_voxel_key(full), _voxel_key(rec))
            assert (_voxel_key(full)[at] == _voxel_key(rec)).all()
            assert (rec["count"] <= full["count"][at]).all()
            assert (wd > 0).sum() > 100_000


def _voxel_key(rec):
    return ((rec["iz"].astype(np.int64) + (1 << 20)) << 42) | \
           ((rec["iy"].astype(np.int64) + (1 << 20)) << 21) | (rec["ix"].astype(np.int64) + (1 << 20))


# ======================================================================= RGB-D ==

PHOTO_FIELDS = -(1 << 31) | ((1 << 26) - 1)      # Y, gx, gy and the valid bit (unpack_photo's fields)
PREP_B = 100


@pytest.mark.parametrize("shape", lf.shapes(3), ids=lf.shape_id)
def test_rgbd_prep_largest_frames(shape, _memory_cap):
    """A: k_rgbd_prep from RGB and from grey: Y, and the photometric word's
    fields (unpack_photo) exact, on a periodic frame (reach: one row)."""
    W, H = shape
    assert lf.admitted(W, H, 3)
    block = lf.rgb_block(PREP_B, W, W + 2 * H)
    if H < PREP_B + 2:
        want = _cuda(lf.photo_words(lf.periodic_frame(block, H, 3)))
    else:
        parts = lf.periodic_truth(lf.photo_words, block, H, 1, 3)
        want = lf.expand(*[_cuda(p) for p in parts], H, 3, index=_cuda(lf.periodic_rows(H, PREP_B, 3)))
    d_in = _periodic_on_device(_cuda(block), H, 3).reshape(1, H, W, 3).contiguous()
    d_gray = torch.full((1, H, W), 7, dtype=torch.uint8, device="cuda")
    d_photo = torch.zeros((1, H, W), dtype=torch.int32, device="cuda")
    d_photo1 = torch.zeros_like(d_photo)
    _ready()
    with youth_rgbd.RgbdContext(W, H, 2) as ctx:
        ctx.prep_device(d_in, 3, 1, d_gray, d_photo)
        ctx.sync()
        ctx.prep_device(d_gray, 1, 1, None, d_photo1)          # the grey path: the same words
        ctx.sync()
        _memory_cap.mark()
    _assert_equal(d_photo[0] & PHOTO_FIELDS, want, "photo words from RGB")
    _assert_equal(d_photo1[0] & PHOTO_FIELDS, want, "photo words from grey")
    _assert_equal(d_gray[0], (want & 255).to(torch.uint8), "Y")
    if H > 2 and W > 2:
        assert int((want < 0).sum()) == (W - 2) * (H - 2)      # the valid bit: all but the border


@pytest.mark.parametrize("shape", lf.shapes(3), ids=lf.shape_id)
def test_rgbd_decimate_largest_frames(shape, _memory_cap):
    """A: k_rgbd_decimate at the stride default_levels picks for the shape (8 on
    the three 2^26-pixel frames, none on the 3-pixel strips) and at the
    smallest and largest strides, 2 and 16."""
    W, H = shape
    picked = [s for s, _ in youth_rgbd.default_levels(W, H) if s > 1]
    assert [(s, 10) for s in picked] == rgbd_levels_truth.default_levels(W, H)[:-1]
    assert picked == ([8] if min(W, H) >= 4096 else [])
    depth = lf.periodic_frame(lf.depth_block(FLT_B, W, 5 + W), H, 1)
    gray = lf.periodic_frame(rgbd_truth.luma(lf.rgb_block(PREP_B, W, H)), H, 2)
    d_depth, d_gray = _cuda(depth[None]), _cuda(gray[None])
    for s in sorted(set(picked) | {2, 16}):
        want_d, want_g = rgbd_levels_truth.decimate(depth, s), rgbd_levels_truth.decimate(gray, s)
        Hs, Ws = want_d.shape
        assert (Hs, Ws) == ((H + s - 1) // s, (W + s - 1) // s)
        od = torch.full((Hs * Ws + 16,), 0x5A5A, dtype=torch.int16, device="cuda")
        og = torch.full((Hs * Ws + 16,), 0x5A, dtype=torch.uint8, device="cuda")
        youth_rgbd.decimate_device(d_depth.data_ptr(), d_gray.data_ptr(), 1, W, H, s, od.data_ptr(),
                                   og.data_ptr())
        _memory_cap.mark()
        _assert_equal(od[:Hs * Ws].view(Hs, Ws), _cuda(want_d), f"depth at stride {s}")
        _assert_equal(og[:Hs * Ws].view(Hs, Ws), _cuda(want_g), f"grey at stride {s}")
        assert (od[Hs * Ws:] == 0x5A5A).all() and (og[Hs * Ws:] == 0x5A).all()


@pytest.mark.parametrize("shape", [(16384, 48), (48, 16384)], ids=lf.shape_id)
def test_rgbd_sums_and_align_on_the_strips(shape, _memory_cap):
    """A: the 31 sums at three poses (counts exact, sums to test_gpu_rgbd.py's
    rtol 1e-11 / atol 1e-9) and a 2-iteration align (the pose within the
    project's 1e-5 of the numpy truth, status and first matches equal)."""
    W, H = shape
    src, dst, _, srgb, drgb = youth_synth.pairs_rgb(11, 1, W, H)
    src, dst = src[0], dst[0]
    sg, dg = rgbd_truth.luma(srgb[0]), rgbd_truth.luma(drgb[0])
    K = oracle.viewer_K(W, H)
    rest = [k for k in range(31) if k not in (28, 30)]
    with youth_rgbd.RgbdContext(W, H, 2, iters=2, lam=0.1) as ctx:
        for T12 in _poses3():
            got = ctx.reduce_host(src, sg, dst, dg, T12)
            want = rgbd_truth.reduce(src, sg, dst, dg, T12, K, 0.10, 0.1)
            assert got[28] == want[28] > 1000 and got[30] == want[30] > 0
            np.testing.assert_allclose(got[rest], want[rest], rtol=1e-11, atol=1e-9)
        d = [_cuda(a[None]) for a in (src, sg, dst, dg)]
        _ready()
        ctx.align_pairs_device(d[0], d[1], d[2], d[3], 1)
        T64, _, st = ctx.poses(1)
        stats = ctx.stats(1)
        _memory_cap.mark()
    T_t, _, st_t, stats_t = rgbd_truth.align(src, sg, dst, dg, K, iters=2, lam=0.1)
    assert st[0] == st_t == 0
    assert np.array_equal(stats[0, 0, [1, 3]], stats_t[0, [1, 3]])
    assert float(np.abs(T64[0, :3] - T_t[:3]).max()) <= 1e-5


def test_rgbd_lambda_zero_is_the_depth_only_align_8192x8192(monkeypatch, _memory_cap):
    """A: at lambda 0 the RGB-D align is the depth-only per-iteration align bit
    for bit (test_gpu_rgbd.py's property) on a 2^26-pixel pair: a 512 x 512
    synthetic pair with every pixel repeated 16 x 16."""
    W = H = 8192
    s, d, _ = youth_synth.pairs(7, 1, W // 16, H // 16)
    up = lambda a: np.repeat(np.repeat(a[0], 16, axis=0), 16, axis=1)[None]
    ds, dd = _cuda(up(s)), _cuda(up(d))
    g = torch.Generator(device="cuda").manual_seed(4)
    gs = torch.randint(0, 256, (1, H, W), generator=g, device="cuda", dtype=torch.uint8)
    gd = torch.randint(0, 256, (1, H, W), generator=g, device="cuda", dtype=torch.uint8)
    monkeypatch.setenv("YOUTH_ICP_NO_COOP", "1")
    monkeypatch.setenv("YOUTH_ICP_NO_PERSISTENT", "1")
    _ready()
    with youth_icp.IcpContext(W, H, 2, iters=2) as icp:
        icp.align_pairs_device(ds.data_ptr(), dd.data_ptr(), 1)
        T_icp, _, st_icp = icp.get_poses(1)
        cnt_icp, r2_icp = icp.get_stats(1, 2)
        assert "per-iteration" in icp.get_plan()["kernel"]
        _memory_cap.mark()
    with youth_rgbd.RgbdContext(W, H, 2, iters=2, lam=0.0) as ctx:
        ctx.align_pairs_device(ds, gs, dd, gd, 1)
        T, _, st = ctx.poses(1)
        stats = ctx.stats(1)
        _memory_cap.mark()
    assert cnt_icp.min() > W * H // 8
    assert np.array_equal(np.ascontiguousarray(T[:, :3]).view(np.uint64),
                          np.ascontiguousarray(T_icp[:, :3]).view(np.uint64))
    assert np.array_equal(st, st_icp)
    assert np.array_equal(stats[:, :, 1].copy().view(np.uint64), cnt_icp.view(np.uint64))
    assert np.array_equal(stats[:, :, 0].copy().view(np.uint64), r2_icp.view(np.uint64))
    assert not stats[:, :, 2].any()
