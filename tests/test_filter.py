"""CPU tests of the edge-preserving depth filter (include/youth_filter.h,
DESIGN.md §11): the numpy restatement (filter_truth.py, the truth of
test_gpu_filter.py) against the known answers of an independent prototype,
the filter's invariants, the exported entry points' argument checks without a
device, and the premise of the whole feature on the C oracle: at SURVEY §8d
noise the filter brings the ICP pose from as wrong as the motion to within
0.05 degrees and 2 mm of the truth."""
import ctypes
import os
import subprocess
import zlib

import numpy as np
import pytest

import oracle
import youth_filter
import youth_icp
import youth_synth
from conftest import PKG, ROOT
from filter_truth import filter_truth, gate

# (pairs index, W, H, flags) of the known-answer frames: the src frame of the pair
KAT_FRAMES = {
    "survey160": (0, 160, 120, youth_synth.SURVEY_FLAGS),
    "default97": (3, 97, 53, youth_synth.DEFAULT_FLAGS),
    "survey24": (5, 24, 16, youth_synth.SURVEY_FLAGS),
}
# frame, (t0, t2) -> crc32 of the int16 output bytes, sum, pixels changed, max |change|
KAT = [
    ("survey160", (8, 96), 0x668CE80E, 47521872, 17068, 31),
    ("survey160", (40, 1000), 0xFFDAB4EB, 47521590, 17542, 56),
    ("default97", (8, 96), 0x751D45C6, 9593505, 2340, 11),
    ("default97", (40, 1000), 0x0ED43947, 9593402, 2547, 28),
    ("survey24", (8, 96), 0x70890C3B, 463328, 293, 5),
    ("survey24", (40, 1000), 0x8484C648, 463337, 310, 6),
]


def kat_frame(name):
    i, W, H, flags = KAT_FRAMES[name]
    return youth_synth.pairs(i, 1, W, H, flags=flags)[0][0]


def hand_case():
    d = np.full((8, 8), 32767, np.int16)
    d[3, 3] = 32600
    d[0, 0] = -5
    d[7, 7] = 0
    return d


def pose_error(T, T_gt):
    """(rotation error in degrees, translation error in mm) of a 4x4 pose."""
    R = T[:3, :3] @ T_gt[:3, :3].T
    ang = np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))
    return float(ang), float(np.linalg.norm(T[:3, 3] - T_gt[:3, 3]) * 1000.0)


@pytest.mark.parametrize("name,params,crc,total,changed,max_change", KAT)
def test_truth_reproduces_the_known_answers(name, params, crc, total, changed, max_change):
    src = kat_frame(name)
    out = filter_truth(src, *params)
    assert out.dtype == np.int16 and out.shape == src.shape
    assert zlib.crc32(out.tobytes()) == crc
    assert int(out.astype(np.int64).sum()) == total
    assert int((out != src).sum()) == changed
    assert int(np.abs(out.astype(np.int64) - src).max()) == max_change


def test_truth_on_the_hand_case():
    """Gate clamped to 255 at depth 32767; an edge of 167 inside it."""
    d = hand_case()
    assert int(gate(32767, 40, 1000)) == 255 and int(gate(32600, 40, 1000)) == 255
    out = filter_truth(d, 40, 1000)
    assert out[3, 3] == 32725 and out[3, 4] == 32759
    assert out[0, 0] == -5 and out[7, 7] == 0
    assert zlib.crc32(out.tobytes()) == 1648779394


@pytest.mark.parametrize("name", sorted(KAT_FRAMES))
def test_identity_validity_and_range(name):
    src = kat_frame(name)
    assert np.array_equal(filter_truth(src, 1, 0), src)
    for t0, t2 in ((8, 96), (40, 1000), (255, 1000)):
        out = filter_truth(src, t0, t2).astype(np.int64)
        assert np.array_equal(out > 0, src > 0)
        v = src > 0
        T = gate(src[v], t0, t2)
        assert (np.abs(out[v] - src[v]) <= T - 1).all()
        assert np.array_equal(out[~v], src[~v])


def test_truth_against_a_python_loop():
    """The vectorised restatement == the definition walked tap by tap."""
    rng = np.random.default_rng(11)
    H, W, t0, t2 = 9, 11, 8, 96
    d = (3000 + rng.integers(-12, 13, size=(H, W))).astype(np.int16)
    d[2, 3] = 0
    d[5, 5] = -7
    d[6, 1] = 3400                        # an edge
    d[0, 10] = 32767
    ws = (1, 2, 4, 2, 1)
    want = d.copy()
    for v in range(H):
        for u in range(W):
            c = int(d[v, u])
            if c <= 0:
                continue
            T = min(255, t0 + ((t2 * (c >> 4) ** 2) >> 16))
            num = den = 0
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if not (0 <= v + dy < H and 0 <= u + dx < W):
                        continue
                    n = int(d[v + dy, u + dx])
                    if n <= 0 or abs(n - c) >= T:
                        continue
                    w = (T * T - (n - c) ** 2) * ws[dy + 2] * ws[dx + 2]
                    den += w
                    num += w * (n - c + T)
            want[v, u] = c - T + (num + (den >> 1)) // den
    assert np.array_equal(filter_truth(d, t0, t2), want)
    # a batch is its frames one by one
    b = np.stack([d, d[::-1].copy(), np.zeros_like(d)])
    got = filter_truth(b, t0, t2)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], filter_truth(b[1], t0, t2))
    assert not got[2].any()


def test_every_declared_filter_symbol_is_exported():
    names = youth_icp.declared_functions(youth_filter.HEADER_PATH)
    assert names == ["youth_depth_filter_default_params", "youth_depth_filter_device",
                     "youth_depth_filter_host", "youth_depth_filter_last_error"]
    icp = youth_icp.declared_functions(os.path.join(ROOT, "include", "youth_icp.h"))
    assert "youth_icp_set_depth_filter" in icp and "youth_icp_get_depth_filter" in icp
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "libyouth_icp.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [n for n in names + ["youth_icp_set_depth_filter", "youth_icp_get_depth_filter"]
                if n not in exported]
    assert youth_filter.default_params() == (8, 96)


def test_filter_header_compiles_as_c99_and_cpp():
    src = ('#include "youth_filter.h"\n'
           'int main(void){youth_filter_params p = {8, 96};\n'
           'return sizeof(p) == 2 * sizeof(int) && p.t0 + p.t2 == 104 ? 0 : 1;}\n')
    for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "c++")):
        r = subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I",
                            os.path.join(ROOT, "include"), "-x", lang, "-"], input=src, text=True,
                           capture_output=True)
        assert r.returncode == 0, r.stderr


def test_bad_arguments_are_refused_before_the_device(has_gpu):
    lib = youth_filter.load_library()
    P = youth_icp.FilterParams
    a = np.zeros(64 * 8, np.int16)
    b = np.zeros(64 * 8, np.int16)
    pa, pb = a.ctypes.data, b.ctypes.data   # never dereferenced: every call below is refused
    E = youth_icp.YOUTH_EINVAL

    def device(*args):
        rc = lib.youth_depth_filter_device(*args)
        return rc, (lib.youth_depth_filter_last_error() or b"").decode()

    for args in ((0, None, pb, 1, 16, 8, None, None),            # NULL in
                 (0, pa, None, 1, 16, 8, None, None),            # NULL out
                 (0, pa, pa, 1, 16, 8, None, None),              # the same buffer
                 (0, pa, pa + 2 * 100, 1, 16, 8, None, None),    # overlapping
                 (0, pa, pb, 1, 2, 8, None, None),               # W = 2
                 (0, pa, pb, 1, 16, 2, None, None),              # H = 2
                 (0, pa, pb, 1, 16385, 8, None, None),
                 (0, pa, pb, 1, 16384, 16384, None, None),       # W*H > 2^26
                 (0, pa, pb, -1, 16, 8, None, None),
                 (0, pa, pb, 65536, 16, 8, None, None),
                 (0, pa, pb, 1, 16, 8, ctypes.byref(P(0, 96)), None),
                 (0, pa, pb, 1, 16, 8, ctypes.byref(P(256, 96)), None),
                 (0, pa, pb, 1, 16, 8, ctypes.byref(P(8, 1001)), None),
                 (0, pa, pb, 1, 16, 8, ctypes.byref(P(8, -1)), None)):
        rc, text = device(*args)
        assert rc == E and "youth_depth_filter_device" in text, (args, rc, text)
    P16 = ctypes.POINTER(ctypes.c_int16)
    ha, hb = a.ctypes.data_as(P16), b.ctypes.data_as(P16)
    assert lib.youth_depth_filter_host(0, None, hb, 1, 16, 8, None) == E
    assert lib.youth_depth_filter_host(0, ha, None, 1, 16, 8, None) == E
    assert lib.youth_depth_filter_host(0, ha, hb, 1, 2, 8, None) == E
    assert lib.youth_depth_filter_host(0, ha, hb, 1, 16, 8, ctypes.byref(P(0, 0))) == E
    assert b"t0" in lib.youth_depth_filter_last_error()
    # the tracker's switch: a null context is refused
    assert lib.youth_icp_set_depth_filter(None, None) == E
    assert lib.youth_icp_get_depth_filter(None, None) == E
    if not has_gpu:
        rc, text = device(0, pa, pb, 1, 16, 8, None, None)
        assert rc == youth_icp.YOUTH_ENODEV and text
        with pytest.raises(youth_icp.IcpError) as e:
            youth_filter.depth_filter_host(a.reshape(8, 64))
        assert e.value.code == youth_icp.YOUTH_ENODEV


def test_accuracy_premise_on_the_oracle():
    """8 pairs at SURVEY noise, 640x480, 10 iterations: filtered, every pair
    is within 0.05 degrees and 2 mm of the generator's T_gt (measured 0.0144
    degrees / 0.83 mm at worst); raw, the median rotation error is >= 0.2
    degrees (measured 0.48)."""
    src, dst, T_gt = youth_synth.pairs(0, 8, 640, 480, flags=youth_synth.SURVEY_FLAGS)
    fs, fd = filter_truth(src), filter_truth(dst)
    raw_rot = []
    for p in range(8):
        T64 = oracle.align(fs[p], fd[p], iters=10)[0]
        rot, trans = pose_error(T64, T_gt[p])
        print(f"pair {p}: filtered {rot:.4f} deg {trans:.3f} mm")
        assert rot <= 0.05 and trans <= 2.0, (p, rot, trans)
        raw_rot.append(pose_error(oracle.align(src[p], dst[p], iters=10)[0], T_gt[p])[0])
    print("raw rotation errors", raw_rot)
    assert float(np.median(raw_rot)) >= 0.2
