"""CPU tests of the removal C-ABI of the voxel map (include/youth_map_remove.h,
reached through youth_map.h):
the new entry points are declared, exported and bound with the signatures of
youth_map.py; NULL maps, NULL outputs and bad sizes are refused before
anything is dereferenced; struct youth_map_stats keeps its size (the new
counters live in a struct of their own).  No device is needed: every refusal
here happens before the first HIP call."""
import ctypes
import os
import subprocess
import sys

import youth_icp
import youth_map
from conftest import PKG, ROOT

LIB = os.path.join(PKG, "libyouth_icp.so")
NEW = ["youth_map_remove_device", "youth_map_remove_host", "youth_map_move_device",
       "youth_map_compact", "youth_map_remove_stats", "youth_slam_map_reintegrate",
       "youth_slam_map_kept"]


def test_new_symbols_are_declared_exported_and_bound():
    declared = youth_icp.declared_functions(youth_map.REMOVE_HEADER_PATH)
    assert sorted(declared) == sorted(NEW)
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = youth_map.load_library()
    for name in NEW:
        assert name in declared and name in exported and name in youth_map._SIGS, name
        fn = getattr(lib, name)
        restype, argtypes = youth_map._SIGS[name]
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes), name
    # the device forms mirror youth_map_integrate_device (move: one pose array more)
    integ = youth_map._SIGS["youth_map_integrate_device"]
    assert youth_map._SIGS["youth_map_remove_device"] == integ
    assert youth_map._SIGS["youth_map_remove_host"] == youth_map._SIGS["youth_map_integrate_host"]
    move = youth_map._SIGS["youth_map_move_device"]
    assert move[0] is integ[0] and move[1] == integ[1][:8] + [ctypes.c_void_p, ctypes.c_void_p]
    for name in ("remove", "remove_device", "move_device", "compact", "remove_stats"):
        assert callable(getattr(youth_map.VoxelMap, name))
    assert callable(youth_map.slam_map_reintegrate) and callable(youth_map.slam_map_kept)


def test_stats_struct_sizes(tmp_path):
    """sizeof(struct youth_map_stats) is ABI: six uint64 as before; the removal
    counters are a second struct of six."""
    src = ('#include <stdio.h>\n#include "youth_map.h"\n'
           'int main(void){printf("%zu %zu %zu\\n", sizeof(struct youth_map_stats),\n'
           ' sizeof(struct youth_map_remove_stats), sizeof(youth_voxel));return 0;}\n')
    exe = str(tmp_path / "sizes")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-", "-o", exe], input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    sizes = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert sizes == ["48", "48", "40"]
    assert ctypes.sizeof(youth_map.MapStats) == 48 and ctypes.sizeof(youth_map.MapRemoveStats) == 48
    assert [n for n, _ in youth_map.MapStats._fields_] == ["integrated", "out_of_range", "dropped",
                                                          "occupied", "direct", "capacity"]
    assert [n for n, _ in youth_map.MapRemoveStats._fields_] == ["removed", "missing", "underflow",
                                                                "live", "vacant", "stale"]


_SWEEP = r"""
import ctypes, sys
import numpy as np
import youth_icp, youth_map
lib = youth_map.load_library()
E = youth_icp.YOUTH_EINVAL
# a readable block stands in for a map where the refusal must come before the
# map is looked at: a dereference would read zeros, not crash, and go on to HIP
fake = ctypes.create_string_buffer(4096)
m = ctypes.cast(fake, ctypes.c_void_p)
d = np.ones(64, np.int16)
dp, dv = d.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), ctypes.c_void_p(d.ctypes.data)
T = np.eye(4).reshape(-1)
Tp = T.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
t32 = np.zeros(12, np.float32)
tv = ctypes.c_void_p(t32.ctypes.data)
st = youth_map.MapRemoveStats()
calls = {
    "remove_device_null_map": lambda: lib.youth_map_remove_device(None, dv, None, 1, 8, 8, None, None, None),
    "remove_device_null_depth": lambda: lib.youth_map_remove_device(m, None, None, 1, 8, 8, None, None, None),
    "remove_host_null_map": lambda: lib.youth_map_remove_host(None, dp, None, 8, 8, None, None),
    "remove_host_null_depth": lambda: lib.youth_map_remove_host(m, None, None, 8, 8, None, None),
    "move_device_null_map": lambda: lib.youth_map_move_device(None, dv, None, 1, 8, 8, None, tv, tv, None),
    "move_device_null_depth": lambda: lib.youth_map_move_device(m, None, None, 1, 8, 8, None, tv, tv, None),
    "move_device_null_old": lambda: lib.youth_map_move_device(m, dv, None, 1, 8, 8, None, None, tv, None),
    "move_device_null_new": lambda: lib.youth_map_move_device(m, dv, None, 1, 8, 8, None, tv, None, None),
    "compact_null_map": lambda: lib.youth_map_compact(None),
    "remove_stats_null_map": lambda: lib.youth_map_remove_stats(None, ctypes.byref(st)),
    "remove_stats_null_out": lambda: lib.youth_map_remove_stats(m, None),
    "reintegrate_negative_n": lambda: lib.youth_slam_map_reintegrate(-1, Tp),
    "reintegrate_null_poses": lambda: lib.youth_slam_map_reintegrate(3, None),
}
for W, H, n in ((0, 8, 1), (8, 0, 1), (-1, 8, 1), (16385, 1, 1), (16384, 8192, 1), (8, 8, -1), (8, 8, 65536)):
    calls[f"remove_device_{W}x{H}x{n}"] = \
        lambda W=W, H=H, n=n: lib.youth_map_remove_device(m, dv, None, n, W, H, None, None, None)
    calls[f"move_device_{W}x{H}x{n}"] = \
        lambda W=W, H=H, n=n: lib.youth_map_move_device(m, dv, None, n, W, H, None, tv, tv, None)
    if n == 1:
        calls[f"remove_host_{W}x{H}"] = \
            lambda W=W, H=H: lib.youth_map_remove_host(m, dp, None, W, H, None, None)
for name, fn in calls.items():
    print(name, fn())
    assert (lib.youth_map_last_error() or b"") != b"" or name.startswith("reintegrate")
# no module is running: nothing kept, nothing to re-integrate
print("kept", lib.youth_slam_map_kept())
print("reintegrate_off", lib.youth_slam_map_reintegrate(1, Tp))
print("reintegrate_zero", lib.youth_slam_map_reintegrate(0, None))
"""


def test_null_maps_null_outputs_and_bad_sizes_are_refused(tmp_path):
    """In the manner of test_abi.py's sweeps: a child process, so that a crash
    fails the test and not the runner."""
    script = tmp_path / "sweep.py"
    script.write_text(_SWEEP)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG] + [p for p in sys.path if p]))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=120,
                       env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = dict(line.split() for line in r.stdout.splitlines())
    zero = {"kept", "reintegrate_off", "reintegrate_zero"}
    assert len(res) >= 13 + 7 * 2 + 5 + 3
    for name, val in res.items():
        assert val == ("0" if name in zero else str(youth_icp.YOUTH_EINVAL)), (name, val)
