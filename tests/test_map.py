"""CPU tests of the voxel map's host side (include/youth_map.h, DESIGN.md
§10): the library exports what the header declares, the derived float form and
the PLY writer on hand-made records, the numpy restatement (map_truth.py, the
truth of test_gpu_map.py) against a plain Python loop, and the behaviour
without a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import youth_icp
import youth_map
from conftest import PKG, ROOT
from map_truth import derived_points, frame_points, restate


def test_every_declared_map_symbol_is_exported():
    names = youth_icp.declared_functions(os.path.join(ROOT, "include", "youth_map.h"))
    assert len(names) == 16, names
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "libyouth_icp.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [n for n in names if n not in exported]
    lib = youth_map.load_library()
    for n in names:
        getattr(lib, n)


def test_map_header_compiles_as_c99_and_cpp():
    src = ('#include "youth_map.h"\n'
           'int main(void){struct youth_map_stats s; youth_voxel v; (void)s; (void)v;\n'
           'return sizeof(youth_voxel) == 40 && sizeof(s) == 48 ? 0 : 1;}\n')
    for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "c++")):
        r = subprocess.run([cc, std, "-Wall", "-Werror", "-fsyntax-only", "-I",
                            os.path.join(ROOT, "include"), "-x", lang, "-"], input=src, text=True,
                           capture_output=True)
        assert r.returncode == 0, r.stderr


def _hand_records():
    rec = np.zeros(4, youth_map.VOXEL_DTYPE)
    #           ix   iy    iz  count  sum_q            sum_c
    rec[0] = (-3, 0, -1048576, 1, (0, 255, 128), (255, 0, 7))
    rec[1] = (-1, -1, -1, 1, (255, 255, 255), (0, 0, 0))
    rec[2] = (0, 5, 100, 3, (3, 300, 765), (30, 301, 765))
    rec[3] = (1048575, -7, 250, 16777215, (16777215 * 255, 1, 0), (16777215 * 255, 16777215, 0))
    return rec


@pytest.mark.parametrize("vpm", [100.0, 4.0, 0.1])
def test_points_on_hand_made_records(vpm):
    rec = _hand_records()
    got = youth_map.points(rec, vpm)
    want = derived_points(rec, vpm)
    assert got.dtype == np.float32 and got.shape == (4, 6)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # count == 1: the point sits at its q cell's centre inside the voxel
    v = float(np.float32(vpm))
    assert got[1, 0] == np.float32((-1 + 255.5 / 256) / v) and got[1, 0] < 0
    assert got[0, 0] == np.float32((-3 + 0.5 / 256) / v)
    assert got[0, 3] == np.float32(1.0) and got[2, 5] == np.float32(1.0)
    with pytest.raises(youth_icp.IcpError) as e:
        youth_map.points(np.zeros(1, youth_map.VOXEL_DTYPE), vpm)      # count 0
    assert e.value.code == youth_icp.YOUTH_EINVAL
    with pytest.raises(youth_icp.IcpError):
        youth_map.points(rec, 0.0)


def test_write_ply_round_trip(tmp_path):
    rec, vpm = _hand_records(), 100.0
    path = str(tmp_path / "m.ply")
    youth_map.write_ply(path, rec, vpm)
    lines = open(path).read().splitlines()
    end = lines.index("end_header")
    head = lines[:end]
    assert head[0] == "ply" and head[1] == "format ascii 1.0"
    assert "element vertex 4" in head
    props = [ln.split()[1:] for ln in head if ln.startswith("property")]
    assert props == [["float", "x"], ["float", "y"], ["float", "z"], ["uchar", "red"],
                     ["uchar", "green"], ["uchar", "blue"], ["uint", "count"]]
    body = lines[end + 1:]
    assert len(body) == 4
    want = derived_points(rec, vpm)
    for k, ln in enumerate(body):                    # one vertex per record, in order
        f = ln.split()
        assert np.array_equal(np.array(f[:3], np.float32), want[k, :3])    # %.9g round-trips
        mean = rec["sum_c"][k].astype(np.float64) / rec["count"][k]
        assert [int(x) for x in f[3:6]] == [int(np.floor(m + 0.5)) for m in mean]
        assert int(f[6]) == rec["count"][k]
    youth_map.write_ply(path, rec[:0], vpm)          # an empty map is a valid file
    assert "element vertex 0" in open(path).read()
    with pytest.raises(youth_icp.IcpError):
        youth_map.write_ply(str(tmp_path / "no_such_dir" / "m.ply"), rec, vpm)


def test_restatement_against_python_loop():
    """The numpy restatement == the definition walked point by point."""
    rng = np.random.default_rng(3)
    W, H, vpm = 5, 7, np.float32(37.5)
    depth = rng.integers(-50, 3000, size=(H, W)).astype(np.int16)
    depth[2, 3] = 0
    rgb = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    T = np.array([[0.0, -1.0, 0.0, 0.3], [1.0, 0.0, 0.0, -0.7], [0.0, 0.0, 1.0, -1.1]], np.float32)
    P, C = frame_points(depth, rgb, None, T)
    assert P.shape[0] == int((depth > 0).sum())
    P = np.vstack([P, np.array([[np.nan, 0, 0], [0, 1e9, 0], [0, 0, -1048576.5 / 37.5],
                                [-1e-30, -0.0, 0.0]], np.float32)])
    C = np.vstack([C, np.full((4, 3), 9, np.uint8)])
    vox, skipped = {}, 0
    for p, c in zip(P, C):
        s = [np.float32(a) * vpm for a in p]
        fl = [np.floor(a) for a in s]
        if not all(-1048576.0 <= a < 1048576.0 for a in fl):
            skipped += 1
            continue
        q = [min(255, int((a - b) * np.float32(256.0))) for a, b in zip(s, fl)]
        r = vox.setdefault(tuple(int(a) for a in fl), [0, [0, 0, 0], [0, 0, 0]])
        r[0] += 1
        r[1] = [x + y for x, y in zip(r[1], q)]
        r[2] = [x + int(y) for x, y in zip(r[2], c)]
    rec, oor = restate(P, C, vpm)
    assert oor == skipped == 3
    keys = sorted(vox, key=lambda k: (k[2], k[1], k[0]))
    assert [tuple(int(x) for x in (r["ix"], r["iy"], r["iz"])) for r in rec] == keys
    for r, k in zip(rec, keys):
        assert int(r["count"]) == vox[k][0]
        assert r["sum_q"].tolist() == vox[k][1] and r["sum_c"].tolist() == vox[k][2]
    # tiny negative s: floor -1, s - fl rounds up to 1.0f, q clamps to 255
    tiny = rec[(rec["ix"] == -1) & (rec["iy"] == 0) & (rec["iz"] == 0)]
    assert tiny.shape[0] == 1 and tiny["sum_q"][0, 0] == 255
    assert int(rec["count"].sum()) == P.shape[0] - 3


def test_map_create_without_a_device_fails_cleanly(has_gpu):
    lib = youth_map.load_library()
    # argument errors come first, with or without a device
    for vpm, slots in ((0.0, 1024), (-1.0, 1024), (float("nan"), 1024), (float("inf"), 1024),
                       (100.0, 0), (100.0, (1 << 28) + 1)):
        with pytest.raises(youth_icp.IcpError) as e:
            youth_map.VoxelMap(vpm, slots)
        assert e.value.code == youth_icp.YOUTH_EINVAL, (vpm, slots)
    assert lib.youth_map_clear(None) == youth_icp.YOUTH_EINVAL
    assert lib.youth_map_voxels(None) == youth_icp.YOUTH_EINVAL
    assert lib.youth_map_extract(None, None, 0) == youth_icp.YOUTH_EINVAL
    assert lib.youth_map_stats(None, None) == youth_icp.YOUTH_EINVAL
    assert lib.youth_map_integrate_host(None, None, None, 4, 4, None, None) == youth_icp.YOUTH_EINVAL
    lib.youth_map_destroy(None)
    # the module's map is off unless YOUTH_SLAM_MAP_VPM was set at init
    assert youth_map.slam_map_voxels() == 0 and youth_map.slam_map_vpm() == 0.0
    assert lib.youth_slam_map_extract(None, 0) == 0
    if not has_gpu:
        with pytest.raises(youth_icp.IcpError) as e:
            youth_map.VoxelMap(100.0)
        assert e.value.code == youth_icp.YOUTH_ENODEV
