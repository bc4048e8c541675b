"""Every instantiation of the ICP core launched against the oracle
(profiles/icp_variants/reach.txt).

icp_kernels.hip compiles k_icp, k_icp_coop, k_reduce, k_prep and k_prep_ident
once per mode (YOUTH_ICP_SPEC fma | survey x YOUTH_ICP_REDUCE exact | lane32:
the kernels' kSp 0..3), division (the verified two-operation one, or IEEE when
YOUTH_ICP_NO_FASTDIV=1 or k_verify_fastdiv refuses the camera) and pixel loop
(aligned: W % 4 == 0, a source base on 8 bytes and centred_exact; else
unaligned).  The rest of the suite runs the default mode's forms; here each
cell of that cube runs on small frames, says which kernel family and form it
ran (get_plan, fastdiv, spec, reduction, get_first_iter, lanes), and is held
to the C oracle in the same spec and reduction (lane32 over the partition the
context reports):

  aligns      status 0 and the oracle's, match counts of every iteration equal
              as integers, sum r^2 within rtol 1e-6, the fp64 pose within
              SAME_VARIANT_TOL = 1e-9, the fp32 device output equal to T32 bit
              for bit;
  stage sums  association indices and the count exact, the 28 sums within rtol
              1e-11 / atol 1e-9; without the association output the same 29
              numbers bit for bit;
  first-iteration forms (exact reductions of k_icp): `identity` equal to
              `general` bit for bit, `prep` (k_prep_ident) within PLAN_TOL =
              1e-12 of it with equal counts and sum r^2 within rtol 1e-9.

Fast against IEEE division, the cell otherwise the same: EVERYTHING an align
or a stage call returns is bit-identical, in every family.  Both divisions
give the same quotients (that is what k_verify_fastdiv admits), so only a
different summation order could move a bit, and none of the orders depends on
the division:
  * k_reduce and k_icp: a chunk's lanes take pixels start + 4 threadIdx.x + q
    (accumulate_chunk), the waves add in fixed order, the chunk's row goes to
    partials[(p nblk + c)] and the pair's last arriver adds the rows in row
    order (handoff_sum, sum_pair_rows).  nblk and chunk come from
    reduce_geometry, which reads the pair count and the concurrency share
    only.  k_icp's grid does come from icp_blocks_per_cu[var], which may
    differ between the two instantiations (run_iterations: `grid = n_cu
    icp_blocks_per_cu[var] / share`), but the grid only decides which
    workgroup dequeues which item (k, p, c), never what an item sums or where
    its row goes: so no plan tolerance is used between the divisions, for
    k_icp either.
  * k_prep_ident: units per frame are blocks_x bands, the band from the batch
    size (launch_prep_ident), rows added by handoff_sum in row order.
  * k_icp_coop: px per lane and threads are forced here, G = ceil(N / (px
    threads)) follows, a workgroup's row is its chunk's.  (What the division
    can change is whether the planner admits the plan, coop_bpc[..][variant 2
    + fast]: each cell asserts the plan it ran.)

Off-8 source and target bases run the unaligned loops and the narrow preps on
W % 4 == 0 frames.  accumulate_chunk gives lane t of a chunk the same four
pixels in both loops (i = start + 4 threadIdx.x; kAligned only changes how the
depth words are loaded and the centred column formed), so the lane32 partition
is by pixel index there too, and every result is compared bit for bit with the
same frames at an aligned base.  The off-centre principal point (the camera of
test_gpu_reduce.test_off_centre_principal_point scaled to 160 columns) takes
the unaligned loop at any base; it is held to the oracle under its own camera,
and at a base off 8 bytes to itself at an aligned one.

A lane32 pose is bounded against its own oracle only: its distance from the
exact one belongs to the data (test_gpu_plans._check).

Inputs: pairs 0..2 of youth_synth.pairs(40, ...), pair 2 started 1 degree / 1
cm off where a T_init is given, 10 iterations.  Under every shape, spec,
reduction and camera used the oracle alone gives status 0 and at least 1000
matches at every iteration of every pair (asserted in _check; smallest: 2523 at
97x53).
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

import oracle
import rgbd_draws
import youth_icp
import youth_synth
from conftest import lanes_of, oracle_like

pytestmark = pytest.mark.gpu
f32 = np.float32
ITERS = 10
N_PAIRS = 3
MIN_MATCHES = 1000
SAME_VARIANT_TOL = 1e-9     # test_gpu_plans / test_gpu_reduce: poses vs the oracle in the same reduction
PLAN_TOL = 1e-12            # test_gpu_ident_first: poses of one align on two launch plans
PERSISTENT = "k_prep + k_icp (persistent)"
PER_ITERATION = "k_prep + k_init + k_reduce x iters (per-iteration)"
MODES = {"fma-exact": ("fma", "exact"), "survey-exact": ("survey", "exact"),
         "fma-lane32": ("fma", "lane32"), "survey-lane32": ("survey", "lane32")}   # kSp 0, 1, 2, 3
SPEC_CODE = {"fma": youth_icp.SPEC_FMA, "survey": youth_icp.SPEC_SURVEY}
REDUCE_CODE = {"exact": youth_icp.REDUCE_EXACT, "lane32": youth_icp.REDUCE_LANE32}
KNOBS = ("YOUTH_ICP_SPEC", "YOUTH_ICP_REDUCE", "YOUTH_ICP_NO_FASTDIV", "YOUTH_ICP_NO_COOP",
         "YOUTH_ICP_NO_PERSISTENT", "YOUTH_ICP_NO_IDENT_FIRST", "YOUTH_ICP_IDENT_FIRST",
         "YOUTH_ICP_COOP_THREADS", "YOUTH_ICP_COOP_PX", "YOUTH_ICP_COOP_TILE_SRC",
         "YOUTH_ICP_QUEUES", "YOUTH_ICP_PREP_BAND", "YOUTH_ICP_COOP_MAX_PAIRS")
FIRST_FORMS = {"general": {"YOUTH_ICP_NO_IDENT_FIRST": "1"}, "identity": {"YOUTH_ICP_IDENT_FIRST": "icp"},
               "prep": {}}
# test_off_centre_principal_point's cx = 20.9316 at W = 640, scaled to 160 columns
OFF_CENTRE_CX = float(f32(20.9316 / 4))
REFUSED = 3     # the camera of rgbd_draws.camera_draws(160, 120) that k_verify_fastdiv refuses

_observed = {"pose": 0.0, "r2": 0.0, "sums": 0.0, "forms": 0.0}


def _report(name):
    print(f"\n[icp variants] {name}: max |pose - oracle| {_observed['pose']:.3e} (bound "
          f"{SAME_VARIANT_TOL:.0e}), max rel sum r^2 error {_observed['r2']:.3e} (1e-6), stage sums "
          f"{_observed['sums']:.3f} of the rtol 1e-11 / atol 1e-9 bar, max |prep - general| "
          f"{_observed['forms']:.3e} (bound {PLAN_TOL:.0e})")


def _err(a, b):
    return float(np.abs(np.asarray(a)[..., :3, :4] - np.asarray(b)[..., :3, :4]).max())


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ------------------------------------------------------------------ inputs --
def _camera(cam, W, H):
    """(the library's intrinsics, the oracle's) of a named camera."""
    if cam == "refused":
        k = rgbd_draws.camera_draws(160, 120)[REFUSED]
        return rgbd_draws.intrinsics(k), oracle.K_of(k)
    K, Ko = youth_icp.default_intrinsics(W, H), oracle.viewer_K(W, H)
    assert K.as_tuple() == (Ko.fx, Ko.fy, Ko.cx, Ko.cy, Ko.depth_scale)
    if cam == "offcentre":
        K.cx = Ko.cx = OFF_CENTRE_CX
    else:
        assert cam == "viewer"
    return K, Ko


def _aligned_loop(cam, W, H, base):
    """run_iterations' and launch_reduce's choice of the pixel loop."""
    return base % 8 == 0 and W % 4 == 0 and rgbd_draws.centred_exact(_camera(cam, W, H)[0].cx, W)


@functools.lru_cache(maxsize=None)
def _inputs(W, H):
    """Pairs 0..2 of youth_synth.pairs(40, n, W, H) and their initial poses:
    identity, but pair 2 starts 1 degree and 1 cm off."""
    src, dst, _ = youth_synth.pairs(40, N_PAIRS, W, H)
    T_init = np.tile(np.eye(4), (N_PAIRS, 1, 1))
    T_init[2] = oracle.se3_exp(np.r_[0.0, np.deg2rad(1.0), 0.0, 0.01, 0.0, 0.0])
    return _frozen(src, dst, T_init)


@functools.lru_cache(maxsize=None)
def _oracle_pair(W, H, cam, spec, lanes, p, init):
    """(T64, status, counts [ITERS], sum r^2 [ITERS]) of pair p from the CPU
    oracle in `spec`: EXACT (lanes None) or LANE32 over the partition `lanes`."""
    src, dst, T_init = _inputs(W, H)
    with oracle.spec(spec), oracle_like(lanes):
        T64, _, st, stats = oracle.align(src[p], dst[p], K=_camera(cam, W, H)[1], iters=ITERS,
                                         T_init=T_init[p] if init else None)
    T64, cnt, r2 = _frozen(T64, stats[:, 0].copy(), stats[:, 1].copy())
    return T64, int(st), cnt, r2


def _device_frames(frames, off):
    """The frames on the device at an int16 element offset `off` from an 8-byte
    boundary, 64 zero elements on either side: (the tensor, the base pointer)."""
    flat = torch.zeros(frames.size + 128, dtype=torch.int16, device="cuda")
    flat[64 + off:64 + off + frames.size] = torch.from_numpy(frames.reshape(-1).copy()).cuda()
    base = flat.data_ptr() + 2 * (64 + off)
    assert base % 8 == 2 * off
    return flat, base


@contextlib.contextmanager
def _knobs(monkeypatch, mode, div, **env):
    """The environment of one cell; every knob is read when a context is created."""
    spec, red = MODES[mode]
    with monkeypatch.context() as mp:
        for k in KNOBS:
            mp.delenv(k, raising=False)
        mp.setenv("YOUTH_ICP_SPEC", spec)
        mp.setenv("YOUTH_ICP_REDUCE", red)
        if div == "ieee":
            mp.setenv("YOUTH_ICP_NO_FASTDIV", "1")
        for k, v in env.items():
            mp.setenv(k, str(v))
        yield


def _align(W, H, cam, init, off=0):
    """A fresh context under the environment as it is, two aligns of the three
    pairs (the arena and counter-set alternation); the second one's results."""
    src, dst, T_init = _inputs(W, H)
    keep_s, d_src = _device_frames(src, off)
    keep_d, d_dst = _device_frames(dst, off)
    out = torch.zeros((N_PAIRS, 16), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with youth_icp.IcpContext(W, H, N_PAIRS, K=_camera(cam, W, H)[0], iters=ITERS) as ctx:
        res = {"fastdiv": ctx.fastdiv, "spec": ctx.spec, "reduction": ctx.reduction,
               "aligned": _aligned_loop(cam, W, H, d_src)}
        for _ in range(2):
            ctx.align_pairs_device(d_src, d_dst, N_PAIRS, T_init=T_init if init else None,
                                   d_T_out=out.data_ptr())
        ctx.sync()
        T64, T32, st = ctx.get_poses(N_PAIRS)
        cnt, r2 = ctx.get_stats(N_PAIRS, ITERS)
        res.update(T64=T64, T32=T32, st=st, cnt=cnt, r2=r2, plan=ctx.get_plan(), lanes=ctx.lanes(),
                   first=ctx.get_first_iter(), Tdev=out.cpu().numpy().reshape(N_PAIRS, 4, 4))
        assert lanes_of(ctx) == (res["lanes"] if res["reduction"] == youth_icp.REDUCE_LANE32 else None)
    del keep_s, keep_d
    return res


def _expect(res, mode, fastdiv, kernel, first, what):
    """No cell passes by running the default: the mode, the division and the
    kernel family and form the context reports."""
    spec, red = MODES[mode]
    assert res["spec"] == SPEC_CODE[spec] and res["reduction"] == REDUCE_CODE[red], what
    assert res["fastdiv"] == fastdiv, (what, res["fastdiv"])
    assert res["plan"]["kernel"] == kernel, (what, res["plan"])
    assert res["first"] == first, (what, res["first"])
    if kernel != "k_icp_coop":
        kind, chunk, threads, _ = res["lanes"]
        assert kind == youth_icp.LANES_STRIDED and threads == 256 and chunk % 1024 == 0, \
            (what, res["lanes"])


def _expect_coop(res, W, H, threads, npx, kind, what):
    G = -(-W * H // (npx * threads))
    assert res["plan"] == {"kernel": "k_icp_coop", "workgroups_per_pair": G, "threads": threads,
                           "px_per_lane": npx}, (what, res["plan"])
    assert res["lanes"] == (kind, npx * threads, threads, npx), (what, res["lanes"])


def _check(res, W, H, cam, mode, init, what):
    """An align against the oracle in the same spec and reduction."""
    spec, red = MODES[mode]
    lanes = res["lanes"] if red == "lane32" else None
    for p in range(N_PAIRS):
        To, sto, cnt_o, r2_o = _oracle_pair(W, H, cam, spec, lanes, p, bool(init and p == 2))
        tag = (what, mode, p)
        assert sto == 0 and cnt_o.min() >= MIN_MATCHES, (tag, sto, cnt_o)    # the inputs' condition
        assert res["st"][p] == sto == 0, (tag, int(res["st"][p]), sto)
        assert np.array_equal(res["cnt"][p], cnt_o), (tag, res["cnt"][p], cnt_o)
        _observed["r2"] = max(_observed["r2"], float(np.abs(res["r2"][p] / r2_o - 1.0).max()))
        np.testing.assert_allclose(res["r2"][p], r2_o, rtol=1e-6, err_msg=str(tag))
        e = _err(res["T64"][p], To)
        _observed["pose"] = max(_observed["pose"], e)
        assert e <= SAME_VARIANT_TOL, (tag, e)
        assert np.array_equal(res["Tdev"][p], res["T32"][p]), tag
        assert res["Tdev"][p, :3].tobytes() == res["T32"][p, :3].tobytes(), tag


def _same_bits(a, b, what):
    for k in ("T64", "T32", "st", "cnt", "r2", "Tdev"):
        assert a[k].tobytes() == b[k].tobytes(), (what, k)
    assert a["lanes"] == b["lanes"] and a["plan"] == b["plan"], what


def _same_align(a, b, what):
    """test_gpu_ident_first's bars between two launch plans of one align."""
    assert np.array_equal(a["st"], b["st"]), what
    assert np.array_equal(a["cnt"], b["cnt"]), (what, np.argwhere(a["cnt"] != b["cnt"])[:4])
    err = float(np.abs(a["T64"] - b["T64"]).max())
    _observed["forms"] = max(_observed["forms"], err)
    assert err <= PLAN_TOL, (what, err)
    np.testing.assert_allclose(a["r2"], b["r2"], rtol=1e-9, err_msg=str(what))


# ------------------------------------------------------------- 1: k_icp --
# name: (W, H, camera, int16 offset of both bases, aligned loop, the loop whose results it repeats)
LOOPS = {
    "aligned-160x120": (160, 120, "viewer", 0, True, None),
    "ragged-97x53": (97, 53, "viewer", 0, False, None),
    "base+2-160x120": (160, 120, "viewer", 1, False, "aligned-160x120"),
    "base+4-160x120": (160, 120, "viewer", 2, False, "aligned-160x120"),
    "offcentre-160x120": (160, 120, "offcentre", 0, False, None),
    "offcentre+2-160x120": (160, 120, "offcentre", 1, False, "offcentre-160x120"),
}
_k_icp_done = {}


def _k_icp_runs(monkeypatch, mode, div, loop):
    """k_icp<mode, div, loop> (YOUTH_ICP_NO_COOP=1): a call with T_init (k_prep,
    the general first iteration) and the identity start in each first-iteration
    form the reduction has, every run checked against the oracle.  Cached: the
    cases at an offset base compare with the aligned one's."""
    key = (mode, div, loop)
    if key in _k_icp_done:
        return _k_icp_done[key]
    W, H, cam, off, aligned, _ = LOOPS[loop]
    exact = MODES[mode][1] == "exact"
    runs = {}
    with _knobs(monkeypatch, mode, div, YOUTH_ICP_NO_COOP=1):
        runs["T_init"] = (_align(W, H, cam, True, off), "general", True)
    for form, env in FIRST_FORMS.items() if exact else [("general", {})]:
        with _knobs(monkeypatch, mode, div, YOUTH_ICP_NO_COOP=1, **env):
            runs["start-" + form] = (_align(W, H, cam, False, off), form, False)
    for name, (res, form, init) in runs.items():
        what = (loop, div, name)
        _expect(res, mode, div == "fast", PERSISTENT, form, what)
        assert res["aligned"] == aligned, what
        _check(res, W, H, cam, mode, init, what)
    _k_icp_done[key] = {name: r[0] for name, r in runs.items()}
    return _k_icp_done[key]


def test_off_centre_camera_selects_the_unaligned_loop():
    """test_off_centre_principal_point's column check at the cx used here: some
    column's (float)u - cx is not ((float)(u & ~3) - cx) + (u & 3), so
    icp_api.cpp's centred_exact refuses the aligned loop at W = 160."""
    cols = np.arange(160)
    cx = f32(OFF_CENTRE_CX)
    assert ((f32(cols) - cx) != ((f32(cols & ~3) - cx) + f32(cols & 3))).any()
    assert not rgbd_draws.centred_exact(OFF_CENTRE_CX, 160)
    assert rgbd_draws.centred_exact(80.0, 160)


@pytest.mark.parametrize("loop", list(LOOPS))
@pytest.mark.parametrize("mode", list(MODES))
def test_k_icp_cube(monkeypatch, mode, loop):
    """The persistent kernel in every mode x division x pixel loop; the
    unaligned loop from a ragged width, from bases 2 and 4 bytes off an 8-byte
    boundary (the target's too: k_prep's narrow form on W % 4 == 0) and from
    the off-centre camera.  Exact reductions run the three first-iteration
    forms (k_prep_ident in its four instantiations).  Between the divisions
    everything is bit-identical (module docstring), and an offset base repeats
    the aligned base's bits."""
    runs = {div: _k_icp_runs(monkeypatch, mode, div, loop) for div in ("fast", "ieee")}
    for name in runs["fast"]:
        _same_bits(runs["fast"][name], runs["ieee"][name], (mode, loop, name, "fast vs ieee"))
    if MODES[mode][1] == "exact":
        for div, r in runs.items():
            _same_bits(r["start-identity"], r["start-general"], (mode, loop, div, "identity"))
            _same_align(r["start-prep"], r["start-general"], (mode, loop, div, "prep"))
    ref = LOOPS[loop][5]
    if ref:
        for div in runs:
            want = _k_icp_runs(monkeypatch, mode, div, ref)
            for name in want:
                _same_bits(runs[div][name], want[name], (mode, loop, div, name, "vs", ref))
    _report(f"k_icp_cube[{mode}-{loop}]")


# -------------------------------------------------------- 2: k_icp_coop --
COOP = {   # name: (W, H, threads, px per lane, tile height)
    "256x24": (128, 48, 256, 6, 24),
    "512x24": (128, 48, 512, 3, 24),
    "512x80": (120, 150, 512, 10, 80),     # ragged on both edges
}


@pytest.mark.parametrize("geom", list(COOP))
@pytest.mark.parametrize("mode", list(MODES))
def test_k_icp_coop_cube(monkeypatch, mode, geom):
    """k_icp_coop<mode, division, threads, tile height> with tile-shaped and
    contiguous source chunks; the 512 / 24 geometry also from bases 2 bytes off
    (the fused prep's narrow form).  Pair 2 starts from its T_init."""
    W, H, threads, npx, th = COOP[geom]
    assert npx * threads == 64 * th and -(-W * H // (npx * threads)) == -(-W // 64) * -(-H // th)
    got = {}
    for div in ("fast", "ieee"):
        for tile_src, off in (("1", 0), ("0", 0)) + ((("1", 1),) if geom == "512x24" else ()):
            with _knobs(monkeypatch, mode, div, YOUTH_ICP_COOP_THREADS=threads, YOUTH_ICP_COOP_PX=npx,
                        YOUTH_ICP_COOP_TILE_SRC=tile_src):
                res = _align(W, H, "viewer", True, off)
            what = (geom, div, tile_src, off)
            _expect(res, mode, div == "fast", "k_icp_coop", "general", what)
            kind = youth_icp.LANES_COOP_TILE if tile_src == "1" else youth_icp.LANES_COOP
            _expect_coop(res, W, H, threads, npx, kind, what)
            _check(res, W, H, "viewer", mode, True, what)
            got[div, tile_src, off] = res
    for (div, tile_src, off), res in got.items():
        _same_bits(res, got["ieee", tile_src, off], (mode, geom, tile_src, off, "fast vs ieee"))
        if off:
            _same_bits(res, got[div, tile_src, 0], (mode, geom, div, "base+2 vs aligned"))
        if MODES[mode][1] == "exact":    # the chunk shape moves the fp64 order only
            assert _err(res["T64"], got[div, "0", 0]["T64"]) <= SAME_VARIANT_TOL
    _report(f"k_icp_coop_cube[{mode}-{geom}]")


# ------------------------------------------------ 3: per-iteration path --
@pytest.mark.parametrize("loop", ["aligned-160x120", "ragged-97x53", "base+2-160x120"])
@pytest.mark.parametrize("mode", list(MODES))
def test_per_iteration_cube(monkeypatch, mode, loop):
    """YOUTH_ICP_NO_COOP=1 YOUTH_ICP_NO_PERSISTENT=1: one fused-solve k_reduce<mode,
    false, division, loop, true> per iteration, its last workgroup solving."""
    W, H, cam, off, aligned, ref = LOOPS[loop]
    got = {}
    for div in ("fast", "ieee"):
        for o in sorted({0, off}) if ref else [off]:
            with _knobs(monkeypatch, mode, div, YOUTH_ICP_NO_COOP=1, YOUTH_ICP_NO_PERSISTENT=1):
                res = _align(W, H, cam, True, o)
            what = (loop, div, o)
            _expect(res, mode, div == "fast", PER_ITERATION, "general", what)
            assert res["aligned"] == (aligned if o == off else True), what
            _check(res, W, H, cam, mode, True, what)
            got[div, o] = res
    for (div, o), res in got.items():
        _same_bits(res, got["ieee", o], (mode, loop, o, "fast vs ieee"))
        _same_bits(res, got[div, 0], (mode, loop, div, "offset vs aligned base"))
    _report(f"per_iteration_cube[{mode}-{loop}]")


# ---------------------------------------------------------- 4: stage sums --
@functools.lru_cache(maxsize=None)
def _stage_poses():
    """The identity and two seeded poses within 4 degrees / 3 cm."""
    rng = np.random.default_rng(0x1A9E)
    poses = [np.eye(4, dtype=f32)[:3]]
    for _ in range(2):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        T = oracle.se3_exp(np.r_[axis * np.deg2rad(rng.uniform(0, 4)), rng.uniform(-0.03, 0.03, 3)])
        poses.append(T[:3].astype(f32))
    return _frozen(*poses)


@pytest.mark.parametrize("W,H", [(160, 120), (97, 53)])
@pytest.mark.parametrize("mode", list(MODES))
def test_stage_sums_cube(monkeypatch, mode, W, H):
    """youth_icp_reduce_host with and without the association output: the
    unfused k_reduce<mode, assoc, division, loop, false>, 32 forms."""
    spec, red = MODES[mode]
    src, dst, _ = _inputs(W, H)
    Ko = oracle.viewer_K(W, H)
    got = {}
    for div in ("fast", "ieee"):
        with _knobs(monkeypatch, mode, div), youth_icp.IcpContext(W, H, 2) as ctx:
            assert ctx.fastdiv == (div == "fast")
            assert ctx.spec == SPEC_CODE[spec] and ctx.reduction == REDUCE_CODE[red]
            for k, T32 in enumerate(_stage_poses()):
                idx, neq = ctx.reduce(src[0], dst[0], T32)
                lanes = ctx.lanes()
                none, neq_only = ctx.reduce(src[0], dst[0], T32, want_assoc=False)
                assert none is None and ctx.lanes() == lanes
                kind, chunk, threads, _ = lanes
                assert kind == youth_icp.LANES_STRIDED and threads == 256 and chunk % 1024 == 0
                assert neq_only.tobytes() == neq.tobytes(), (div, k)
                with oracle.spec(spec), oracle_like(ctx):
                    want = oracle.reduce(src[0], dst[0], T32, Ko)
                    want_idx = oracle.associate(src[0], dst[0], T32, Ko)
                assert want[28] >= MIN_MATCHES, (k, want[28])
                assert np.array_equal(idx, want_idx), (div, k)
                assert neq[28] == want[28] == (idx >= 0).sum(), (div, k, neq[28], want[28])
                frac = float((np.abs(neq - want) / (1e-9 + 1e-11 * np.abs(want))).max())
                _observed["sums"] = max(_observed["sums"], frac)
                np.testing.assert_allclose(neq, want, rtol=1e-11, atol=1e-9, err_msg=str((div, k)))
                got[div, k] = (idx, neq)
    for k in range(3):
        assert np.array_equal(got["fast", k][0], got["ieee", k][0]), k
        assert got["fast", k][1].tobytes() == got["ieee", k][1].tobytes(), k
    _report(f"stage_sums_cube[{mode}-{W}x{H}]")


# --------------------------- 5: a camera the context itself refuses --
def _fmaf(a, b, c):
    """RN(a b + c) in float32, elementwise: the product of two float32 is exact
    in fp64; the fp64 sum is made round-to-odd (TwoSum gives the sign of what
    the addition lost), which the rounding to float32 cannot see."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(np.asarray(c, np.float64), p.shape)
    s = p + c
    bb = s - p
    lost = (p - (s - bb)) + (c - bb)
    odd = (s.view(np.int64) & 1) != 0
    s = np.where((lost != 0) & ~odd, np.nextafter(s, np.where(lost > 0, np.inf, -np.inf)), s)
    return s.astype(f32)


def _fast_consts(y):
    """icp_api.cpp fast_consts: h = RN(1 / y), l = RN((1 - y h) / y)."""
    y = f32(y)
    h = f32(1.0) / y
    resid = _fmaf(np.array([-y]), np.array([h]), f32(1.0))[0]
    return h, f32(np.float64(resid) / np.float64(y))


@functools.lru_cache(maxsize=None)
def _fastdiv_mismatches(k, W, H):
    """k_verify_fastdiv on the host: mismatches of div_fast(n, h, l) = fma(n, h,
    n l) against n / y over d in [1, 32767], u in [0, W), v in [0, H)."""
    fx, fy, cx, cy, ds = (f32(v) for v in k)
    d = np.arange(1, 32768).astype(f32)
    zi = d / ds
    h, l = _fast_consts(ds)
    bad = int((_fmaf(d, np.broadcast_to(h, d.shape), d * l) != zi).sum())
    for n_px, c, f in ((W, cx, fx), (H, cy, fy)):
        h, l = _fast_consts(f)
        n = (np.arange(n_px).astype(f32)[:, None] - c) * zi[None, :]
        bad += int((_fmaf(n, np.broadcast_to(h, n.shape), n * l) != n / f).sum())
    return bad


@pytest.mark.parametrize("mode", list(MODES))
def test_camera_the_context_refuses(monkeypatch, mode):
    """No knob: the context's own k_verify_fastdiv refuses camera 3 of
    rgbd_draws.camera_draws(160, 120) (5 mismatches on the host, the check's
    arithmetic restated above; centred, so the aligned loops stay) and admits
    camera 0.  The IEEE kernels of the persistent, cooperative and
    per-iteration families on that verdict, against the oracle under the
    camera."""
    W, H = 160, 120
    cams = rgbd_draws.camera_draws(W, H)
    assert _fastdiv_mismatches(cams[REFUSED], W, H) == 5 and _fastdiv_mismatches(cams[0], W, H) == 0
    assert rgbd_draws.centred_exact(cams[REFUSED][2], W)
    with _knobs(monkeypatch, mode, "own"):
        with youth_icp.IcpContext(W, H, 2, K=rgbd_draws.intrinsics(cams[0])) as ctx:
            assert ctx.fastdiv
        with youth_icp.IcpContext(W, H, 2, K=rgbd_draws.intrinsics(cams[REFUSED])) as ctx:
            assert not ctx.fastdiv
    exact = MODES[mode][1] == "exact"
    cells = [("k_icp T_init", {"YOUTH_ICP_NO_COOP": 1}, True, PERSISTENT, "general"),
             ("k_icp start", {"YOUTH_ICP_NO_COOP": 1}, False, PERSISTENT, "prep" if exact else "general"),
             ("coop", {"YOUTH_ICP_COOP_PX": 3}, True, "k_icp_coop", "general"),
             ("per-iteration", {"YOUTH_ICP_NO_COOP": 1, "YOUTH_ICP_NO_PERSISTENT": 1}, True,
              PER_ITERATION, "general")]
    for name, env, init, kernel, first in cells:
        with _knobs(monkeypatch, mode, "own", **env):
            res = _align(W, H, "refused", init)
        _expect(res, mode, False, kernel, first, name)
        assert res["aligned"], name
        if kernel == "k_icp_coop":
            _expect_coop(res, W, H, 512, 3, youth_icp.LANES_COOP, name)
        _check(res, W, H, "refused", mode, init, name)
    _report(f"camera_the_context_refuses[{mode}]")
