"""Input recipes and non-vacuity counters of test_gpu_limits.py (the side units
at the frame, batch and table limits they accept); numpy and the truth
modules only, pinned without a GPU by test_limits.py.

Three recipes keep the CPU truth of a 2^26-pixel frame affordable while every
output element is still compared:

* periodic frames for the local operators (depth filter, RGB-D prep and
  decimation): the frame is vertical repeats of one block of rows, so the
  truth of the block with its wrapped halo is the truth of every row further
  than the operator's reach from the frame's top and bottom, and two thin
  strips give those (`periodic_frame`, `periodic_truth`, `expand`);
* sparse validity for the units whose cost follows the valid pixels (viewer
  cloud, voxel map, renderer): `sparse_pixels` always holds the frame's four
  corner pixels in raster order and the first pixel of the last tile;
* many tiny frames as one frame for the 65535-frame batches
  (`stack_with_gaps`, `tile_parts`, `signature_20x15`), each pinned to the
  per-frame truth.
"""
import numpy as np

import rectify_truth
import rgbd_truth
import youth_rgbd

MAX_SIDE = 16384
MAX_PIXELS = 1 << 26
MAX_FRAMES = 65535          # kMaxFrames = the hardware limit of gridDim.y
BIG = [(8192, 8192), (16384, 4096), (4096, 16384)]


def shapes(min_w, min_h=None):
    """The (W, H) of cases A for a unit whose smallest frame is min_w x min_h."""
    min_h = min_w if min_h is None else min_h
    return BIG + [(MAX_SIDE, min_h), (min_w, MAX_SIDE)]


def shape_id(s):
    return f"{s[0]}x{s[1]}"


def admitted(W, H, min_w, min_h=None):
    """hip_host.h's frame_size_ok."""
    min_h = min_w if min_h is None else min_h
    return min_w <= W <= MAX_SIDE and min_h <= H <= MAX_SIDE and W * H <= MAX_PIXELS


# ------------------------------------------------------------ periodic frames --

def periodic_rows(H, B, phase=0):
    """Row y of the frame is row (y + phase) % B of the block."""
    return (np.arange(H, dtype=np.int64) + phase) % B


def periodic_frame(block, H, phase=0):
    return block[periodic_rows(H, block.shape[0], phase)]


def periodic_interior(truth, block, halo):
    """The truth of the block's rows far from the frame's border: the block
    with `halo` wrapped rows above and below, those rows cut off again."""
    B = block.shape[0]
    assert halo >= 1 and B >= 2 * halo
    wrapped = block[np.arange(-halo, B + halo) % B]
    return truth(wrapped)[halo:halo + B]


def periodic_truth(truth, block, H, halo, phase=0, interior=None):
    """The truth of periodic_frame(block, H, phase) under a row-local operator:
    `truth` maps rows [h][...] to h rows of output, row y depending on input
    rows y - halo .. y + halo (fewer at the frame's border) and not on y
    itself.  Returns (interior [B], top [halo], bottom [halo]): see expand.
    The interior does not depend on H or the phase and may be passed in."""
    B = block.shape[0]
    assert H >= 4 * halo
    if interior is None:
        interior = periodic_interior(truth, block, halo)
    rows = periodic_rows(H, B, phase)
    top = truth(block[rows[:2 * halo]])[:halo]
    bottom = truth(block[rows[H - 2 * halo:]])[halo:]
    return interior, top, bottom


def expand(interior, top, bottom, H, phase=0, index=None):
    """The expected frame of periodic_truth's parts.  numpy arrays by default;
    torch tensors with index = the periodic_rows as a tensor on their device."""
    halo = top.shape[0]
    rows = periodic_rows(H, interior.shape[0], phase) if index is None else index
    out = interior[rows]
    out[:halo] = top
    out[H - halo:] = bottom
    return out


def depth_block(B, W, seed):
    """B rows of depth that keep the filter's gate busy: a slope with small
    noise, steps, holes, negatives and a band near the int16 ceiling."""
    rng = np.random.default_rng(seed)
    x = np.arange(W, dtype=np.int64)[None, :]
    y = np.arange(B, dtype=np.int64)[:, None]
    d = 900 + (x * 7 + y * 3) % 2600 + rng.integers(-6, 7, (B, W))
    d = np.where((x // 97 + y // 11) % 5 == 0, d + 400, d)
    d[:, W // 3:W // 3 + 9] = 32700 + rng.integers(-60, 68, (B, min(9, W - W // 3)))
    d[rng.random((B, W)) < 0.08] = 0
    d[rng.random((B, W)) < 0.02] = -9
    return d.astype(np.int16)


# ------------------------------------------------------------ sparse validity --

def last_tile_first_pixel(N, tile_px):
    return (N - 1) // tile_px * tile_px


def sparse_pixels(W, H, n, seed, tile_px=(1024, 2048)):
    """Sorted flat indices of about n valid pixels of a W x H frame: the first
    and last pixel, the last of the first row, the first of the last row, the
    first pixel of the last tile (at each tile size) and random ones."""
    N = W * H
    rng = np.random.default_rng(seed)
    must = [0, N - 1, W - 1, (H - 1) * W] + [last_tile_first_pixel(N, t) for t in tile_px]
    idx = np.unique(np.concatenate([np.asarray(must, np.int64),
                                    rng.integers(0, N, min(n, N), dtype=np.int64)]))
    return idx


def sparse_counters(idx, W, H, tile_px):
    """What a sparse case is for: the corners present, the last tile reached
    (and whether it is partial), the scan's run length R = ceil(tiles / 256)."""
    N = W * H
    tiles = (N + tile_px - 1) // tile_px
    s = set(int(i) for i in (0, N - 1, W - 1, (H - 1) * W))
    have = set(int(i) for i in idx[np.isin(idx, list(s))])
    last0 = last_tile_first_pixel(N, tile_px)
    return {"corners": have == s, "tiles": tiles, "R": (tiles + 255) // 256,
            "last_tile_valid": int(((idx >= last0) & (idx < N)).sum()),
            "last_tile_partial": N % tile_px != 0}


def sparse_depth(W, H, idx, seed):
    """int16 [H][W]: depth > 0 at idx, 0 or negative elsewhere (both invalid)."""
    rng = np.random.default_rng(seed)
    d = np.zeros(W * H, np.int16)
    d[1::5003] = -3                       # negatives are invalid too
    d[idx] = rng.integers(400, 9000, idx.size).astype(np.int16)
    return d.reshape(H, W)


def sparse_rgb(W, H, idx, seed):
    """uint8 [H][W][3]: random at idx, 0 elsewhere (never read into a vertex)."""
    rng = np.random.default_rng(seed + 1)
    c = np.zeros((W * H, 3), np.uint8)
    c[idx] = rng.integers(0, 256, (idx.size, 3)).astype(np.uint8)
    return c.reshape(H, W, 3)


# ----------------------------------------------------- offsets past 32 bits --

def last_frame_offset(n_frames, frame_bytes):
    """The byte offset of the last frame of a batch in its array."""
    return (n_frames - 1) * frame_bytes


def smallest_batch_past_32_bits(frame_bytes):
    """The smallest n whose last frame's byte offset no longer fits 32 bits."""
    return -(-(1 << 32) // frame_bytes) + 1


def batch_kinds(n):
    """The frame kind of each frame of a case-B batch: 0 the first, 1 the
    identical middle, 2 and 3 the last two.  A wrapped offset lands on a frame
    of another kind."""
    assert n >= 4
    k = np.ones(n, np.int64)
    k[0], k[n - 2], k[n - 1] = 0, 2, 3
    return k


# ------------------------------------------------- 65535 tiny frames as one --

def counter_depth(n, H, W):
    """n different H x W depth frames from a counter: pixel p of frame f holds
    1 + (f * H * W + p) % 8191 (small enough that the 3 x 3 neighbours pass
    each other's gate now and then), every 7th value 0, every 11th negative."""
    c = np.arange(n * H * W, dtype=np.int64)
    d = 1 + (c * 37) % 8191
    d[c % 7 == 3] = 0
    d[c % 11 == 5] = -4
    return d.reshape(n, H, W).astype(np.int16)


def stack_with_gaps(frames, gap):
    """[n][H][W] -> one frame [n * (H + gap)][W], `gap` rows of 0 after every
    frame.  Under the depth filter a 0 never contributes and is copied, the
    same as a cell outside the frame, so with gap >= 2 the filter's truth of
    the stack is the stack of the frames' truths (`unstack`)."""
    n, H, W = frames.shape
    out = np.zeros((n, H + gap, W), frames.dtype)
    out[:, :H] = frames
    return out.reshape(n * (H + gap), W)


def unstack(stacked, n, H, gap):
    W = stacked.shape[1]
    return np.ascontiguousarray(stacked.reshape(n, H + gap, W)[:, :H])


def tile_parts(parts, n):
    """rectify_truth.map_parts of one W x H frame -> the parts of n such frames
    side by side ([H][n * W]): each copy's taps stay inside its own copy, since
    ix <= W - 2."""
    cov, ix, iy, a, b = parts
    W = cov.shape[1]
    off = (np.arange(n, dtype=np.int64) * W).repeat(W)[None, :]
    t = lambda p: np.tile(p, (1, n))
    return t(cov), np.where(t(cov), t(ix) + off, 0), t(iy), t(a), t(b)


def side_by_side(frames):
    """[n][H][W]... -> [H][n * W]..."""
    n, H, W = frames.shape[:3]
    return np.ascontiguousarray(np.moveaxis(frames, 0, 1).reshape((H, n * W) + frames.shape[3:]))


def from_side_by_side(wide, n):
    H, nW = wide.shape[:2]
    return np.ascontiguousarray(np.moveaxis(wide.reshape((H, n, nW // n) + wide.shape[2:]), 1, 0))


def signature_20x15(depth, gray):
    """loop_truth.signature of 20 x 15 frames, where a pixel is a cell (n = 1):
    the record is depth | gray << 16 | 1 << 31 for depth > 0, gray << 16
    otherwise.  [n][15][20] -> uint32 [n][300]."""
    d = np.asarray(depth).astype(np.int64).reshape(-1, 300)
    y = np.asarray(gray).astype(np.int64).reshape(-1, 300)
    return np.where(d > 0, d | (y << 16) | (1 << 31), y << 16).astype(np.uint32)


# ------------------------------------------------ voxel-map key and table edges --

BOUNDARY_VPM = float(1 << 20)      # 21-bit cells: -2^20 .. 2^20 - 1 span [-1 m, 1 m)
CELL_MIN, CELL_MAX = -(1 << 20), (1 << 20) - 1


def boundary_points():
    """Hand-made world points for a map of 2^20 voxels per metre, as
    (P [n][3] float32, cls [n] of str):

    corner    the eight corner cells: every axis -1.0 (cell -2^20) or
              nextafter(1, 0) (cell 2^20 - 1, q = 240);
    near      in range, an fp32 step inside the two faces;
    out       out of range on exactly one axis: 1.0 or nextafter(-1, -2);
    ordinary  well inside, two of them twice (count 2)."""
    f = np.float32
    lo, hi = f(-1.0), np.nextafter(f(1.0), f(0.0))
    out_hi, out_lo = f(1.0), np.nextafter(f(-1.0), f(-2.0))
    in_lo, in_hi = np.nextafter(lo, f(0.0)), np.nextafter(hi, f(0.0))
    pts, cls = [], []
    for z in (lo, hi):
        for y in (lo, hi):
            for x in (lo, hi):
                pts.append((x, y, z))
                cls.append("corner")
    for k in range(3):
        p = [f(0.5), f(-0.25), f(0.125)]
        p[k], p[(k + 1) % 3] = in_lo, in_hi
        pts.append(tuple(p))
        cls.append("near")
    for k in range(3):
        for o in (out_hi, out_lo):
            p = [f(0.25), f(-0.5), hi]
            p[k] = o
            pts.append(tuple(p))
            cls.append("out")
    rng = np.random.default_rng(8)
    plain = rng.uniform(-0.9, 0.9, (6, 3)).astype(f)
    for p in list(plain) + [plain[0], plain[3]]:
        pts.append(tuple(p))
        cls.append("ordinary")
    return np.array(pts, f), np.array(cls)


def point_frames(P):
    """One 1 x 1 frame per point, its pose all translation (the linear part 0):
    the kernel's fma chain fma(0, z, fma(0, y, fma(0, x, p))) is p exactly.
    -> (depth [n][1][1] int16, rgb [n][1][1][3] uint8, T [n][12] float32)."""
    n = P.shape[0]
    depth = (1000 + np.arange(n)).astype(np.int16).reshape(n, 1, 1)
    rgb = (np.arange(n * 3, dtype=np.int64) * 41 % 256).astype(np.uint8).reshape(n, 1, 1, 3)
    T = np.zeros((n, 3, 4), np.float32)
    T[:, :, 3] = P
    return depth, rgb, T.reshape(n, 12)


def distinct_voxel_frame(n, seed=0):
    """A 1-row frame of n pixels at depth 1 m under the camera
    (1, 1, 0, 0, 1000): pixel u is the world point (u, 0, 1), so at 1 voxel
    per metre and coarser every pixel is its own voxel.
    -> (depth [1][n] int16, rgb [1][n][3] uint8, camera tuple)."""
    rng = np.random.default_rng(seed)
    return (np.full((1, n), 1000, np.int16), rng.integers(0, 256, (1, n, 3)).astype(np.uint8),
            (1.0, 1.0, 0.0, 0.0, 1000.0))


# the renderer's queue: k_map_render_splat takes 1024 slots per workgroup
QUEUE_SLOTS = 1024
QUEUE_VPM = 1000.0
QUEUE_K_IN = (50.0, 50.0, 80.0, 60.0, 5000.0)       # the camera the cluster is integrated with
QUEUE_K_VIEW = (570.0, 570.0, 1024.0, 1024.0, 5000.0)
QUEUE_VIEW = (2048, 2048)


def queue_frame(seed=6):
    """160 x 120 pixels 10 to 36 mm in front of a wide camera: about 19 000
    different 1-mm voxels, many times what a 1024-slot table holds, all nearer
    than fx / (15 vpm) = 38 mm of the view camera, where a footprint is 16 x 16.
    -> (depth, rgb)."""
    rng = np.random.default_rng(seed)
    return (rng.integers(50, 181, (120, 160)).astype(np.int16),
            rng.integers(0, 256, (120, 160, 3)).astype(np.uint8))


def queue_counters(u0, v0, s, n_records, W, H):
    """How many of the table's voxels survive the culls, with a 16 x 16
    footprint wholly inside the frame."""
    whole = (s == 16) & (u0 >= 0) & (v0 >= 0) & (u0 + 16 <= W) & (v0 + 16 <= H)
    return {"records": int(n_records), "survivors": int(u0.size), "whole_16x16": int(whole.sum())}


# ------------------------------------------------------ RGB-D prep, rectifier --

def photo_words(rgb_rows):
    """The packed photometric words of RGB rows [h][W][3], from the truth's Y
    and gradients: unpack_photo's layout, int32 bit patterns."""
    Y = rgbd_truth.luma(rgb_rows)
    gx, gy, valid = rgbd_truth.photo_record(Y)
    w = Y.astype(np.int64) | ((gx + 255).astype(np.int64) << 8) | ((gy + 255).astype(np.int64) << 17) \
        | (valid.astype(np.int64) << 31)
    w = w.astype(np.uint32)
    back = youth_rgbd.unpack_photo(w)
    assert np.array_equal(back[0], Y) and np.array_equal(back[1], gx) and np.array_equal(back[2], gy) \
        and np.array_equal(back[3], valid)
    return w.view(np.int32)


def rgb_block(B, W, seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 256, (B, W, 3), dtype=np.uint8)
    c[:, W // 2] = 0
    c[:, min(W // 2 + 1, W - 1)] = 255             # the largest gradient
    c[B // 2] = 255
    return c


def identity_map_holds(W, H, K):
    """Without distortion the rectifier's map is separable: us depends on u
    alone and vs on v alone (rad is exactly 1, tx and ty exactly 0).  One row
    and one column of the truth show every source position equal to its pixel
    under the camera K = (fx, fy, cx, cy, ds)."""
    fx, fy, cx, cy, ds = K
    zero = (0.0, 0.0, 0.0, 0.0, 0.0)
    us, _ = rectify_truth.source_position(W, 2, K, zero, (fx, fy, cx, 0.0, ds))
    _, vs = rectify_truth.source_position(2, H, K, zero, (fx, fy, 0.0, cy, ds))
    return bool(np.array_equal(us[0], np.arange(W, dtype=np.float32)) and
                np.array_equal(vs[:, 0], np.arange(H, dtype=np.float32)))
