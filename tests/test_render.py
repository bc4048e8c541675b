"""CPU tests of the map render (include/youth_map_render.h): the
numpy restatement (render_truth.py, the truth of test_gpu_render.py) against a
plain Python double loop, the host-only pose rule, the exported symbols, and
the synthetic-scene property of the definition itself."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import youth_icp
import youth_map
import youth_synth
from conftest import PKG, ROOT
from map_truth import restate_frames
from render_truth import render, view_from_pose

F = np.float32


def test_every_declared_render_symbol_is_exported():
    names = youth_icp.declared_functions(os.path.join(ROOT, "include", "youth_map_render.h"))
    assert names == ["youth_map_render_device", "youth_map_render_host",
                     "youth_map_view_from_pose", "youth_slam_map_render"]
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "libyouth_icp.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [n for n in names if n not in exported]
    lib = youth_map.load_library()
    for n in names:
        getattr(lib, n)


def test_render_header_compiles_as_c99_and_cpp_through_either_include():
    body = ('int main(void){struct youth_map_view v = {16, 12, 0, 0};\n'
            'int (*f)(const double*, float*) = youth_map_view_from_pose;\n'
            'int (*g)(youth_map*) = youth_map_clear; (void)f; (void)g;\n'
            'return sizeof(v) == 16 ? 0 : 1;}\n')
    for first in ("youth_map.h", "youth_map_render.h"):
        for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "c++")):
            r = subprocess.run([cc, std, "-Wall", "-Werror", "-fsyntax-only", "-I",
                                os.path.join(ROOT, "include"), "-x", lang, "-"],
                               input=f'#include "{first}"\n' + body, text=True, capture_output=True)
            assert r.returncode == 0, r.stderr


# ------------------------------------------------------------ the pose rule --
def _pose(seed, t_scale=3.0):
    rng = np.random.default_rng(seed)
    w = rng.normal(size=3)
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    T[:3, 3] = rng.normal(size=3) * t_scale
    return T


def test_view_from_pose_is_the_fp64_rule():
    for seed in range(6):
        T = _pose(seed)
        V = youth_map.view_from_pose(T)
        assert V.dtype == np.float32 and V.shape == (3, 4)
        want = np.zeros((3, 4), np.float32)
        for r in range(3):
            for c in range(3):
                want[r, c] = F(T[c, r])
            want[r, 3] = F(-((T[0, r] * T[0, 3] + T[1, r] * T[1, 3]) + T[2, r] * T[2, 3]))
        assert np.array_equal(V.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(V.view(np.uint32), view_from_pose(T).view(np.uint32))
        assert np.array_equal(V, youth_map.view_from_pose(T[:3]))          # 3x4 accepted
        # it is the inverse: V * T = identity to fp32
        assert np.abs(V.astype(np.float64) @ T - np.eye(4)[:3]).max() < 1e-5
    assert np.array_equal(youth_map.view_from_pose(np.eye(4)), np.eye(4, dtype=np.float32)[:3])


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 1e200])
def test_view_from_pose_rejects_non_finite(bad):
    for at in ((0, 0), (1, 2), (2, 3)):
        T = _pose(1)
        T[at] = bad
        with pytest.raises(youth_icp.IcpError) as e:
            youth_map.view_from_pose(T)
        assert e.value.code == youth_icp.YOUTH_EINVAL
    lib = youth_map.load_library()
    assert lib.youth_map_view_from_pose(None, None) == youth_icp.YOUTH_EINVAL
    assert b"view_from_pose" in lib.youth_map_last_error()


def test_render_entry_points_reject_a_null_map():
    lib = youth_map.load_library()
    view = youth_map.MapView(16, 12, 0, 0)
    assert lib.youth_map_render_host(None, ctypes.byref(view), None, None, None, None) == youth_icp.YOUTH_EINVAL
    assert lib.youth_map_render_device(None, 1, ctypes.byref(view), None, None, None, None, None) == \
        youth_icp.YOUTH_EINVAL
    # the module keeps no map unless YOUTH_SLAM_MAP_VPM was set at init
    assert youth_map.slam_map_render(16, 12) is None


# ------------------------------------------- the truth against a plain loop --
def _hand_records():
    """About 40 records around a camera at the origin looking along +z, vpm 50:
    near and far, behind, at the borders, ties, heavy and single-point voxels."""
    rng = np.random.default_rng(11)
    rows = []
    for k in range(30):
        cnt = int(rng.integers(1, 6))
        rows.append((int(rng.integers(-30, 30)), int(rng.integers(-22, 22)),
                     int(rng.integers(-20, 160)), cnt,
                     tuple(int(x) for x in rng.integers(0, 255 * cnt + 1, 3)),
                     tuple(int(x) for x in rng.integers(0, 255 * cnt + 1, 3))))
    rows += [
        (0, 0, 1, 1, (0, 0, 128), (9, 9, 9)),              # z = 0.03 m: the max_splat clamp
        (0, 0, 0, 1, (0, 0, 0), (1, 2, 3)),                # z ~ 0: d rounds to 0
        (3, 2, 50, 2, (20, 20, 20), (200, 100, 50)),       # two on one pixel: the nearer wins
        (3, 2, 50, 0, (0, 0, 0), (0, 0, 0)),               # placeholder, replaced below
        (6, 4, 100, 1, (0, 0, 0), (10, 20, 30)),
        (-40, 0, 50, 3, (30, 30, 30), (0, 0, 0)),          # left of the frame, inside the margin
        (0, -30, 50, 3, (30, 30, 30), (0, 0, 0)),          # above
        (1048575, 0, 50, 1, (255, 255, 255), (255, 255, 255)),
        (0, 0, 2000, 1, (0, 0, 0), (5, 5, 5)),             # 40 m: d > 32767
        (0, 0, -50, 4, (0, 0, 0), (7, 7, 7)),              # behind
    ]
    rec = np.zeros(len(rows), youth_map.VOXEL_DTYPE)
    for k, r in enumerate(rows):
        rec[k] = r
    # the same centroid depth and pixel as the voxel before, another colour: a tie on d
    rec[33] = (3, 2, 50, 2, (20, 20, 20), (200, 100, 48))
    return rec


def _loop_render(rec, vpm, V, K, W, H, max_splat, min_count):
    vpm = F(vpm)
    fx, fy, cx, cy, ds = (F(a) for a in K.as_tuple())
    V = np.asarray(V, np.float32)
    z = [[None] * W for _ in range(H)]
    for r in rec:
        n = int(r["count"])
        if n < min_count:
            continue
        p = []
        for a, name in enumerate(("ix", "iy", "iz")):
            c = F(F(int(r["sum_q"][a])) / F(n))
            p.append(F(F(F(int(r[name])) + F(F(c + F(0.5)) * F(0.00390625))) / vpm))
        with np.errstate(all="ignore"):
            cam = [F(F(F(F(V[q, 0] * p[0]) + F(V[q, 1] * p[1])) + F(V[q, 2] * p[2])) + V[q, 3])
                   for q in range(3)]
            xc, yc, zc = cam
            if not zc > 0:
                continue
            d = F(np.rint(F(zc * ds)))
            if not 1 <= d <= 32767:
                continue
            uf = F(F(F(xc * fx) / zc) + cx)
            vf = F(F(F(yc * fy) / zc) + cy)
            if not (-32 < uf < W + 32 and -32 < vf < H + 32):
                continue
            q = F(fx / F(vpm * zc))
        s = max_splat if math.isinf(q) else max(1, min(max_splat, int(math.ceil(float(q)))))
        h = F(F(0.5) * F(s - 1))
        u0 = int(math.floor(float(F(F(uf - h) + F(0.5)))))
        v0 = int(math.floor(float(F(F(vf - h) + F(0.5)))))
        col = [(int(r["sum_c"][j]) + n // 2) // n for j in range(3)]
        val = (int(d) << 24) | (col[0] << 16) | (col[1] << 8) | col[2]
        for y in range(max(v0, 0), min(v0 + s, H)):
            for x in range(max(u0, 0), min(u0 + s, W)):
                if z[y][x] is None or val < z[y][x]:
                    z[y][x] = val
    depth = np.zeros((H, W), np.int16)
    rgb = np.zeros((H, W, 3), np.uint8)
    for y in range(H):
        for x in range(W):
            if z[y][x] is not None:
                depth[y, x] = z[y][x] >> 24
                rgb[y, x] = [(z[y][x] >> 16) & 255, (z[y][x] >> 8) & 255, z[y][x] & 255]
    return depth, rgb


@pytest.mark.parametrize("max_splat,min_count", [(16, 1), (1, 1), (3, 2)])
def test_restatement_against_python_loop(max_splat, min_count):
    rec = _hand_records()
    assert 35 <= rec.shape[0] <= 45
    K = youth_icp.Intrinsics(20.0, 21.0, 8.0, 6.0, 1000.0)
    W, H, vpm = 16, 12, 50.0
    views = [np.eye(4, dtype=np.float32)[:3], view_from_pose(_pose(3, 0.3)),
             view_from_pose(np.array([[0, 0, 1, -1.0], [0, 1, 0, 0.1], [-1, 0, 0, 1.5]], float))]
    covered = 0
    for V in views:
        got_d, got_c = render(rec, vpm, V, K, W, H, max_splat, min_count)
        want_d, want_c = _loop_render(rec, vpm, V, K, W, H, max_splat, min_count)
        assert got_d.dtype == np.int16 and got_c.dtype == np.uint8
        assert np.array_equal(got_d, want_d) and np.array_equal(got_c, want_c)
        assert (got_c[got_d == 0] == 0).all()
        covered += int((got_d > 0).sum())
    assert covered >= 8
    # the named cases, at the identity view
    d, c = render(rec, vpm, views[0], K, W, H, max_splat, min_count)
    assert d.shape == (H, W) and c.shape == (H, W, 3)
    # z = 0.03 m alone: s = ceil(20 / (50 * 0.03004)) = 14, clamped by max_splat,
    # centred on (8, 6) and clipped to the 12 rows
    for m, area in ((16, 14 * 12), (3, 9), (1, 1)):
        near = render(rec[30:31], vpm, views[0], K, W, H, m, 1)[0]
        assert (near == 30).sum() == area and (near[near > 0] == 30).all() and near[6, 8] == 30
    # the tie on d at one pixel: the smaller packed colour (blue 24) wins
    tie = render(rec[32:34], vpm, views[0], K, W, H, 1, 1)
    assert (tie[0] > 0).sum() == 1 and tie[1][tie[0] > 0].tolist() == [[100, 50, 24]]
    # min_count removes the single-point voxels
    assert (render(rec[rec["count"] == 1], vpm, views[0], K, W, H, 16, 2)[0] == 0).all()


# --------------------------------------------- the synthetic-scene property --
SCENE_K = (142.575, 142.575, 80.0, 60.0, 1000.0)


def scene_case():
    """The case of the issue's 160x120 row: frames 0-3 and 5-7 of the synthetic
    sequence at their ground-truth poses into a map of 100 voxels per metre;
    the view at pose 4 against the clean render there.  Returns the frames'
    (depth, None, K, T32) list, K, T_wc[4] and the clean frame."""
    K = youth_icp.Intrinsics(*SCENE_K)
    frames, T_wc = youth_synth.sequence(0, 8, 160, 120, K)
    T32 = T_wc.reshape(8, 16)[:, :12].astype(np.float32).reshape(8, 3, 4)
    used = [(frames[f], None, K, T32[f]) for f in (0, 1, 2, 3, 5, 6, 7)]
    clean = youth_synth.render(T_wc[4], 160, 120, K, flags=0)
    return used, K, T_wc[4], clean


def scene_figures(depth, clean):
    valid = clean > 0
    cov = (depth > 0) & valid
    err = np.abs(depth.astype(np.int32) - clean.astype(np.int32))[cov]
    return {"coverage": cov.sum() / valid.sum(),
            "ghost": ((depth > 0) & ~valid).sum() / depth.size,
            "median": float(np.median(err)), "p90": float(np.percentile(err, 90))}


def test_synthetic_scene_property_of_the_definition():
    """Conditions on the definition, not on a kernel: the bounds stand a little
    above the figures a numpy prototype of the definition gave for this scene
    (coverage 0.9905, nothing covered where the clean render is invalid,
    median 0 mm, p90 1 mm)."""
    used, K, T4, clean = scene_case()
    rec, oor = restate_frames(used, 100.0)
    assert oor == 0
    depth, rgb = render(rec, 100.0, view_from_pose(T4), K, 160, 120)
    fig = scene_figures(depth, clean)
    print(fig)
    assert fig["coverage"] >= 0.98
    assert fig["ghost"] <= 0.005
    assert fig["median"] <= 2 and fig["p90"] <= 5
    assert (rgb == 0).all()                              # a colourless map
