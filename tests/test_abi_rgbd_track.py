"""CPU tests of the C-ABI the streaming RGB-D tracker adds (include/youth_rgbd.h:
youth_rgbd_track_*, youth_rgbd_pull_host; include/youth_icp.h:
youth_slam_rgbd_active): declared means exported, NULL for every pointer
argument is refused without a dereference, and the headers stay C99 and C++."""
import ctypes
import os
import subprocess
import sys

import youth_icp
import youth_rgbd
from conftest import PKG, ROOT

LIB = os.path.join(PKG, "libyouth_icp.so")
NEW_RGBD = ["youth_rgbd_track_set_batch", "youth_rgbd_track_set_depth_filter",
            "youth_rgbd_track_submit", "youth_rgbd_track_collect", "youth_rgbd_track_pending",
            "youth_rgbd_track_reset", "youth_rgbd_pull_host"]
NEW_ICP = ["youth_slam_rgbd_active"]


def test_new_functions_are_declared_exported_and_bound():
    rgbd = youth_icp.declared_functions(os.path.join(ROOT, "include", "youth_rgbd.h"))
    icp = youth_icp.declared_functions(os.path.join(ROOT, "include", "youth_icp.h"))
    assert set(NEW_RGBD) <= set(rgbd) and set(NEW_ICP) <= set(icp)
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    missing = [n for n in rgbd + NEW_ICP if n not in exported]
    assert not missing, missing
    # the Python mirrors know every one of them
    assert set(rgbd) <= set(youth_rgbd._SIGS)
    lib = youth_rgbd.load_library()
    for n in NEW_RGBD + NEW_ICP:
        assert getattr(lib, n).argtypes is not None


_NULL_SWEEP = r"""
import ctypes, re, sys
text = open(sys.argv[1]).read()
text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
text = re.sub(r"typedef[^;]*;", "", text)
lib = ctypes.CDLL(sys.argv[2])
for ret, name, args in re.findall(r"\n\s*([A-Za-z_][\w ]*?\**)\s*\b(youth_\w+)\(([^;{]*)\)\s*;", text):
    if not name.startswith(("youth_rgbd_track_", "youth_rgbd_pull_host")) or name.endswith("host_sequence"):
        continue
    n = " ".join(args.split()).count(",") + 1
    f = getattr(lib, name)
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p] * n
    print(name, f(*([None] * n)), flush=True)
lib.youth_slam_rgbd_active.restype = ctypes.c_int
print("youth_slam_rgbd_active", lib.youth_slam_rgbd_active(), flush=True)
lib.youth_rgbd_last_error.restype = ctypes.c_char_p
print("text", (lib.youth_rgbd_last_error() or b"").decode().replace(" ", "_"), flush=True)
"""


def test_null_arguments_are_refused_not_dereferenced(tmp_path):
    """All-NULL calls in a child process, so a crash fails the test and not the
    runner: every one returns YOUTH_EINVAL (pending: 0) and leaves a text."""
    script = tmp_path / "sweep.py"
    script.write_text(_NULL_SWEEP)
    r = subprocess.run([sys.executable, str(script), os.path.join(ROOT, "include", "youth_rgbd.h"),
                        LIB], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = dict(line.split() for line in r.stdout.splitlines())
    assert set(NEW_RGBD + NEW_ICP) <= set(res), sorted(res)
    einval = str(youth_icp.YOUTH_EINVAL)
    for n in NEW_RGBD:
        assert res[n] == ("0" if n == "youth_rgbd_track_pending" else einval), (n, res[n])
    assert res["youth_slam_rgbd_active"] == "0"          # no module running
    assert "null_context" in res["text"]


def test_headers_compile_as_c99_and_cpp():
    src = ('#include "youth_rgbd.h"\n#include "youth_icp.h"\n#include "youth_filter.h"\n'
           'int main(void){return youth_rgbd_track_pending(0) + youth_slam_rgbd_active();}\n')
    inc = os.path.join(ROOT, "include")
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++11")):
        r = subprocess.run([cc, std, "-Wall", "-Werror", "-fsyntax-only", "-I", inc, "-x",
                            "c" if cc == "gcc" else "c++", "-"], input=src, text=True,
                           capture_output=True)
        assert r.returncode == 0, r.stderr
