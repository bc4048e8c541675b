"""CPU tests of the measurement tools the round-5 findings rest on
(tools/slam_trace.py): a synthetic event trace in slam_rate's format, with
one slow submission, is summarised per pass as DESIGN.md §6 quotes it."""
import os
import subprocess
import sys

from conftest import ROOT


def test_slam_trace_summary_names_the_slow_submission(tmp_path):
    ev = [(0.0000, 1, 0), (0.0001, 2, 0), (0.0002, 3, 1), (0.0002, 4, 1), (0.0003, 12, 1),
          (0.0003, 12, 2), (0.0004, 12, 3), (0.0004, 12, 4), (0.0005, 12, 5), (0.0005, 5, 0),
          (0.0006, 3, 8), (0.0006, 4, 8), (0.0007, 12, 1), (0.0007, 12, 2), (0.0090, 12, 3),
          (0.0091, 12, 4), (0.0092, 12, 5), (0.0092, 5, 0), (0.0093, 6, 2), (0.0095, 7, 1)]
    p = tmp_path / "events.txt"
    p.write_text("# pass 0 100.000000000 100.010000000\n" +
                 "".join(f"{t + 100.0:.9f} {k} {a}\n" for t, k, a in ev))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "slam_trace.py"), str(p)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout
    assert "pass 0:" in out and "launches 2" in out
    assert "slow submit of 8 frames" in out and "step 3 +8.400" in out
    assert "longest call submit 8.600 ms" in out


def test_kernel_reach_reports_the_unreached_set(tmp_path):
    """tools/kernel_reach.py on a hand-written name list and two hand-written
    stats CSVs: full demangled names as rocprofv3 writes them, a labelled file
    and one with a Test column, a foreign kernel, a zero-call row."""
    (tmp_path / "names.txt").write_text(
        "# unit name\n"
        "rectify k_rectify_map\n"
        "rectify void k_rectify<true, true>\n"
        "rectify k_rectify<true, false>\n"
        "rectify k_rectify<false, true>\n"
        "viewer_cloud k_cloud_scan\n"
        "icp_kernels k_icp<2, false>\n")
    (tmp_path / "a.csv").write_text(
        '"Name","Calls","TotalDurationNs"\n'
        '"void (anonymous namespace)::k_rectify<true, false>((anonymous namespace)::RectCam, uint2 const*, int)",3,10\n'
        '"(anonymous namespace)::k_rectify_map((anonymous namespace)::RectCam, uint2*, int, int)",2,10\n'
        '"__amd_rocclr_copyBuffer",55,10\n'
        '"void (anonymous namespace)::k_rectify<false, true>((anonymous namespace)::RectCam)",0,0\n')
    (tmp_path / "b.csv").write_text(
        '"Test","Name","Calls"\n'
        '"tests/t.py::test_one","k_cloud_scan(int const*, int, int*, int*)",4\n'
        '"tests/t.py::test_two","k_cloud_scan(int const*, int, int*, int*)",1\n'
        '"tests/t.py::test_two","void (anonymous namespace)::k_rectify<true, false>((anonymous namespace)::RectCam)",1\n')
    (tmp_path / "notes.txt").write_text("k_icp<2, false>\tYOUTH_ICP_PX=2 on an unaligned width\n")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "kernel_reach.py"), "--names",
           str(tmp_path / "names.txt"), "--notes", str(tmp_path / "notes.txt"),
           f"tests/test_a.py={tmp_path / 'a.csv'}", str(tmp_path / "b.csv")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = [ln.split("\t") for ln in r.stdout.splitlines() if not ln.startswith("#")]
    assert lines == [
        ["rectify", "k_rectify_map", "2", "tests/test_a.py"],
        ["rectify", "k_rectify<true, true>", "0", "-"],
        ["rectify", "k_rectify<true, false>", "4", "tests/test_a.py"],
        ["rectify", "k_rectify<false, true>", "0", "-"],
        ["viewer_cloud", "k_cloud_scan", "5", "tests/t.py::test_one"],
        ["icp_kernels", "k_icp<2, false>", "0", "-", "YOUTH_ICP_PX=2 on an unaligned width"]]
    assert "# 6 instantiations, 3 without a launch" in r.stdout
    unreached = {ln[1] for ln in lines if ln[2] == "0"}
    assert unreached == {"k_rectify<true, true>", "k_rectify<false, true>", "k_icp<2, false>"}
    # --require: an unreached kernel of a named unit is an error, of another unit none
    assert subprocess.run(cmd + ["--require", "rectify"], capture_output=True, timeout=60).returncode == 1
    assert subprocess.run(cmd + ["--require", "viewer_cloud"], capture_output=True, timeout=60).returncode == 0
