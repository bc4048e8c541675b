"""GPU checks of the identity-pose first iteration (icp_device.h
ident_accumulate, DESIGN.md §2 "the identity lemma").

An align without T_init starts every pair at the identity pose, where each
source pixel matches the target record at its own index, so iteration 0
needs no transform, projection or gather.  Three forms ("mode" below):

  off   YOUTH_ICP_NO_IDENT_FIRST=1: the general iteration 0, the reference;
  icp   YOUTH_ICP_IDENT_FIRST=icp: k_icp runs the identity form on the same
        lanes in the same order, so EVERYTHING the align returns is
        bit-identical to `off`: poses, statuses, per-iteration statistics;
  prep  the default: iteration 0 runs inside the target prep pass
        (k_prep_ident) with its own summation order: poses within 1e-12 of
        `off` (the bar DESIGN.md sets between launch plans) and POSE_TOL of
        the oracle, match counts equal as integers at every iteration,
        statuses equal, iteration 0's sum of squares within rtol 1e-11 /
        atol 1e-9 of the oracle's at the identity pose.

Also the degenerate inputs, and that every call the form does not cover (a
T_init, the lane32 reduction, the small-batch and per-iteration kernels, the
stage call that stores X/Y/Z planes) reports and runs the general form.
"""
import numpy as np
import pytest
import torch

import oracle
import youth_icp
import youth_synth

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-5
PLAN_TOL = 1e-12            # poses of one align on two launch plans
MODES = {"off": {"YOUTH_ICP_NO_IDENT_FIRST": "1"}, "icp": {"YOUTH_ICP_IDENT_FIRST": "icp"},
         "prep": {}}
FORM = {"off": "general", "icp": "identity", "prep": "prep"}
SHAPES = [(97, 53, 3), (161, 122, 2), (640, 480, 2)]   # W % 4 != 0 (unaligned loop); odd; aligned
SPECS = ["survey", "fma"]


def _align(monkeypatch, src, dst, *, mode, spec="survey", iters=10, T_init=None, reduction=None,
           env=(("YOUTH_ICP_NO_COOP", "1"),), sequence=False):
    """One device align in a fresh context (the knobs are read at create):
    -> dict of poses, statuses, stats, the plan and the first iteration's form."""
    for k, v in env:
        monkeypatch.setenv(k, v)
    for k in ("YOUTH_ICP_NO_IDENT_FIRST", "YOUTH_ICP_IDENT_FIRST"):
        monkeypatch.delenv(k, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    n, H, W = src.shape
    ds = torch.from_numpy(src).cuda()
    dd = torch.from_numpy(dst).cuda() if dst is not None else None
    torch.cuda.synchronize()
    with youth_icp.IcpContext(W, H, max(n, 2), iters=iters, spec=spec, reduction=reduction) as ctx:
        if sequence:
            ctx.align_sequence_device(ds.data_ptr(), n)
            n -= 1
        else:
            ctx.align_pairs_device(ds.data_ptr(), dd.data_ptr(), n, T_init=T_init)
        ctx.sync()
        T64, T32, st = ctx.get_poses(n)
        cnt, r2 = ctx.get_stats(n, iters)
        return {"T64": T64, "T32": T32, "st": st, "cnt": cnt, "r2": r2,
                "plan": ctx.get_plan()["kernel"], "first": ctx.get_first_iter()}


def _same_bits(a, b, what):
    for k in ("T64", "T32", "st", "cnt", "r2"):
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _same_align(a, b, what):
    """Two launch plans of one align: summation order only."""
    assert np.array_equal(a["st"], b["st"]), what
    assert np.array_equal(a["cnt"], b["cnt"]), (what, np.argwhere(a["cnt"] != b["cnt"])[:4])
    err = float(np.abs(a["T64"] - b["T64"]).max())
    assert err <= PLAN_TOL, (what, err)
    np.testing.assert_allclose(a["r2"], b["r2"], rtol=1e-9, err_msg=str(what))


def _three(monkeypatch, src, dst, what, **kw):
    """The align in all three modes: forms as reported, icp == off bit for
    bit, prep == off up to summation order.  -> (prep, off)."""
    res = {m: _align(monkeypatch, src, dst, mode=m, **kw) for m in ("off", "icp", "prep")}
    for m, r in res.items():
        assert r["first"] == FORM[m], (what, m, r["first"])
        assert r["plan"].startswith("k_prep + k_icp") and r["plan"] == res["off"]["plan"]
    _same_bits(res["icp"], res["off"], what)
    _same_align(res["prep"], res["off"], what)
    return res["prep"], res["off"]


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("W,H,n", SHAPES)
def test_identity_first_iteration_is_bit_identical(W, H, n, spec, monkeypatch):
    src, dst, _ = youth_synth.pairs(40, n, W, H)
    on, off = _three(monkeypatch, src, dst, (W, H, spec), spec=spec)
    assert not on["st"].any() and (on["cnt"] > 1000).all()
    with oracle.spec(spec):
        To, sto, stats = oracle.align_batch(src, dst, K=oracle.viewer_K(W, H), iters=10,
                                            n_threads=n, want_stats=True)
    assert np.array_equal(on["st"], sto)
    assert np.array_equal(on["cnt"], stats[..., 0])          # match counts, every iteration
    err = float(np.abs(on["T64"][:, :3] - To[:, :3]).max())
    assert err <= POSE_TOL, err
    # iteration 0's sums against the oracle at the identity pose
    eye = np.eye(4, dtype=np.float32)[:3]
    for p in range(n):
        with oracle.spec(spec):
            neq = oracle.reduce(src[p], dst[p], eye, oracle.viewer_K(W, H))
        assert on["cnt"][p, 0] == neq[28]
        np.testing.assert_allclose(on["r2"][p, 0], neq[27], rtol=1e-11, atol=1e-9)


@pytest.mark.parametrize("iters", [1, 2])
def test_short_aligns(iters, monkeypatch):
    """iters = 1: the identity iteration is also the last one (its solve
    writes the output poses); iters = 2: one general iteration follows."""
    src, dst, _ = youth_synth.pairs(41, 3, 97, 53)
    on, off = _three(monkeypatch, src, dst, iters, iters=iters)
    To, sto = oracle.align_batch(src, dst, K=oracle.viewer_K(97, 53), iters=iters, n_threads=3)
    assert np.array_equal(on["st"], sto)
    assert float(np.abs(on["T64"][:, :3] - To[:, :3]).max()) <= POSE_TOL


def test_many_pairs_on_eight_queues(monkeypatch):
    """130 pairs: from 128 pairs up k_icp pulls its items from eight queues."""
    src, dst, _ = youth_synth.pairs(42, 130, 97, 53)
    on, off = _three(monkeypatch, src, dst, 130)
    To, sto = oracle.align_batch(src, dst, K=oracle.viewer_K(97, 53), iters=10, n_threads=16)
    assert np.array_equal(on["st"], sto)
    assert float(np.abs(on["T64"][:, :3] - To[:, :3]).max()) <= POSE_TOL


def test_sequence(monkeypatch):
    """A 33-frame sequence (frame k + 1 aligned to frame k: 32 pairs whose
    sources and targets are the same frames, the last frame no pair's target)."""
    frames, _ = youth_synth.sequence(43, 33, 97, 53)
    on, off = _three(monkeypatch, frames, None, "sequence", sequence=True)
    assert not on["st"].any()
    To, sto = oracle.align_batch(frames[1:], frames[:-1], K=oracle.viewer_K(97, 53), iters=10,
                                 n_threads=16)
    assert np.array_equal(on["st"], sto)
    assert float(np.abs(on["T64"][:, :3] - To[:, :3]).max()) <= POSE_TOL


def test_degenerate_inputs(monkeypatch):
    """An all-zero source or target (FEW_MATCHES at iteration 0, the pose stays
    identity) and a single fronto-parallel plane (DEGENERATE): status and pose
    as on the general path and as the oracle gives them."""
    W, H = 97, 53
    src, dst, _ = youth_synth.pairs(44, 3, W, H)
    src, dst = src.copy(), dst.copy()
    src[0] = 0                       # no valid source pixel
    dst[1] = 0                       # no target record
    src[2] = dst[2] = 1500           # one plane: rank-deficient normal equations
    on, off = _three(monkeypatch, src, dst, "degenerate")
    assert np.array_equal(on["T64"], off["T64"])
    To, sto = oracle.align_batch(src, dst, K=oracle.viewer_K(W, H), iters=10, n_threads=3)
    assert np.array_equal(on["st"], sto)
    assert on["st"][0] == on["st"][1] == youth_icp.STATUS_FEW_MATCHES
    assert on["st"][2] == youth_icp.STATUS_DEGENERATE
    assert np.array_equal(on["T64"], np.broadcast_to(np.eye(4), (3, 4, 4)))
    assert (on["cnt"][:2] == 0).all()


def test_uncovered_calls_keep_the_general_form(monkeypatch):
    """A T_init (even the identity matrix itself), the lane32 reduction, the
    cooperative small-batch kernel and the per-iteration path run and report
    the general form; their results do not depend on the knob."""
    W, H, n = 97, 53, 3
    src, dst, _ = youth_synth.pairs(45, n, W, H)
    Ti = np.broadcast_to(np.eye(4), (n, 4, 4)).copy()
    Ti[1, :3, 3] = (0.004, -0.002, 0.003)
    cases = {
        "T_init": dict(T_init=Ti),
        "lane32": dict(reduction="lane32"),
        "coop": dict(env=()),
        "per_iteration": dict(env=(("YOUTH_ICP_NO_COOP", "1"), ("YOUTH_ICP_NO_PERSISTENT", "1"))),
    }
    for name, kw in cases.items():
        with monkeypatch.context() as mp:
            on = _align(mp, src, dst, mode="prep", **kw)
        with monkeypatch.context() as mp:
            off = _align(mp, src, dst, mode="off", **kw)
        assert (on["first"], off["first"]) == ("general", "general"), name
        assert on["plan"] == off["plan"], name
        _same_bits(on, off, name)
    # the stage call that stores X/Y/Z planes beside the records: k_prep as it was
    planes = []
    for mode in ("prep", "off"):
        with monkeypatch.context() as mp:
            for k, v in MODES[mode].items():
                mp.setenv(k, v)
            with youth_icp.IcpContext(W, H, 2) as ctx:
                planes.append(ctx.prepare(dst[0], want_xyz=True))
                assert ctx.get_first_iter() == "general"
    for a, b in zip(*planes):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    # and the covered call next to them, in the same terms
    with monkeypatch.context() as mp:
        assert _align(mp, src, dst, mode="prep")["first"] == "prep"
