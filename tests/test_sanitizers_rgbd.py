"""Race and memory checks of the SLAM module's RGB-D worker (slam_api.cpp with
YOUTH_SLAM_RGBD=1): tests/tsan_rgbd/rgbd_driver.cpp, a
stand-alone program, drives processSlamFrame with depth and colour from several
threads, resets, size changes and stops with a backlog, built with
-fsanitize=thread and with -fsanitize=address,undefined.  The device entry
points come from tests/tsan/icp_stub.c, the RGB-D tracker from
tests/tsan_rgbd/rgbd_stub.cpp (a CPU stand-in of the hook table whose poses are
a function of the frames' bytes), so it runs without a GPU.  Host code only;
nothing is preloaded and nothing is loaded into Python.
"""
import fcntl
import os
import platform
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
TSAN = os.path.join(HERE, "tsan_rgbd")


@pytest.fixture(scope="module")
def drivers():
    with open(os.path.join(TSAN, ".build.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-C", TSAN, "-j2"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail("sanitizer build failed:\n" + r.stdout + r.stderr)
    return TSAN


def _run(drivers, kind, env):
    """ThreadSanitizer needs its fixed shadow mappings: where setarch can switch
    address randomisation off for a child, the tsan driver runs under it
    (tests/test_sanitizers.py)."""
    cmd = [os.path.join(drivers, "rgbd_driver_" + kind)]
    setarch = shutil.which("setarch")
    if kind == "tsan" and setarch:
        fixed = [setarch, platform.machine(), "-R"]
        if subprocess.run(fixed + ["true"], capture_output=True).returncode == 0:
            cmd = fixed + cmd
    env_all = {k: v for k, v in os.environ.items() if not k.startswith("YOUTH_SLAM_")}
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300, env={**env_all, **env})


TSAN_ENV = {"TSAN_OPTIONS": "halt_on_error=1 second_deadlock_stack=1"}
ASAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1 abort_on_error=0",
            "UBSAN_OPTIONS": "halt_on_error=1 print_stacktrace=1"}


@pytest.mark.parametrize("kind,env", [
    ("tsan", TSAN_ENV), ("asan", ASAN_ENV),
    ("tsan", {**TSAN_ENV, "YOUTH_SLAM_TRACK_BATCH": "1"}),
    ("asan", {**ASAN_ENV, "YOUTH_SLAM_TRACK_BATCH": "3"}),
], ids=["tsan", "asan", "tsan-batch1", "asan-batch3"])
def test_rgbd_worker_under_sanitizer(drivers, kind, env):
    r = _run(drivers, kind, env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "rgbd worker: all scenarios passed" in out
    assert "RGB-D tracking" in out          # the module did start in RGB-D mode
    for marker in ("ThreadSanitizer", "AddressSanitizer", "LeakSanitizer", "runtime error"):
        assert marker not in out, out[-4000:]
