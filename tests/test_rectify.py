"""CPU tests of the lens rectifier (include/youth_rectify.h):
the numpy restatement against an independent fp64 evaluation of the model, the
identity at D = 0, the YAML's distortion keys, the distorted synthetic source,
the NULL-argument sweep of the header, and what the feature is for: tracking
distorted frames with and without the rectifier."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import rectify_truth as rt
import rgbd_truth
import youth_icp
import youth_rectify
import youth_synth
from conftest import GOLDEN, PKG, ROOT

K160 = (142.575, 142.575, 80.0, 60.0, 1000.0)
D_BARREL = (-0.28, 0.07, 8e-4, -6e-4, 0.0)
D_PINCUSHION = (0.20, -0.05, -1e-3, 5e-4, 0.01)
K97 = (90.0, 117.0, 47.3, 26.6, 1000.0)            # fy / fx = 1.3, fractional principal point
# name -> (W, H, K, D, Ko)
CAMERAS = {
    "barrel160": (160, 120, K160, D_BARREL, None),
    "pincushion160": (160, 120, K160, D_PINCUSHION, None),
    "ragged97": (97, 53, K97, (-0.2, 0.05, 1e-3, -5e-4, 0.01), None),
    "tiny2x2": (2, 2, (3.0, 3.0, 0.7, 0.6, 1000.0), D_BARREL, None),
    "tiny4x3": (4, 3, (5.0, 5.5, 1.6, 1.2, 1000.0), D_BARREL, None),
    "wide_ko160": (160, 120, K160, D_BARREL, (0.8 * 142.575, 0.8 * 142.575, 80.0, 60.0, 1000.0)),
}

# The value of the feature: sixteen C5 frames at 160x120 under
# K160, tracked frame to frame with rgbd_truth at lambda = 0.1 (the first lap's
# near-frontal wall leaves depth-only ICP 6.7 degrees off on the ideal frames
# already, §13), D = D_BARREL.  Measured: e_ideal 0.1202 deg / 3.76 mm, e_rect
# 0.0535 deg / 1.81 mm, e_raw 2.42 deg / 121 mm.  The bound is 4 x e_ideal,
# rounded up (§13's convention for a bound over a measured value).
VALUE_ROT_DEG = 0.5
VALUE_TRANS_MM = 16.0


def intr(K):
    return youth_icp.Intrinsics(*[float(v) for v in K])


def hostile_depth(W, H, seed=3):
    """Holes, -1, -32768, 32767 and a checkerboard of valid and invalid
    pixels around a smooth surface."""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:H, 0:W]
    d = (1500 + 3 * u + 2 * v + rng.integers(-4, 5, size=(H, W))).astype(np.int16)
    d[rng.random((H, W)) < 0.05] = 0
    d[rng.random((H, W)) < 0.02] = -1
    d[rng.random((H, W)) < 0.01] = -32768
    d[rng.random((H, W)) < 0.01] = 32767
    h, w = H // 3, W // 3
    board = ((u + v) & 1).astype(bool)[:h, :w]
    d[:h, :w] = np.where(board, d[:h, :w], 0)
    return d


# ------------------------------------------------------------------- truth --

@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_truth_map_against_fp64(name):
    """The fixed-point source position is the fp64 model's to 1/64 px (the
    rounding to 1/32 px) plus the fp32 evaluation's error: at most 12
    roundings of 2^-24 relative on magnitudes <= 256 px, 1.9e-4 px."""
    W, H, K, D, Ko = CAMERAS[name]
    eps = 12 * 256 * 2.0 ** -24
    cov, ix, iy, a, b = rt.map_parts(W, H, K, D, Ko)
    us, vs = rt.source_position_f64(W, H, K, D, Ko)
    err = np.maximum(np.abs(ix + a / 32.0 - us), np.abs(iy + b / 32.0 - vs))
    print(name, "covered", int(cov.sum()), "max error px", float(err[cov].max(initial=0)))
    assert (err[cov] <= 1 / 64 + eps).all()
    inside = (us >= eps) & (us <= W - 1 - eps) & (vs >= eps) & (vs <= H - 1 - eps)
    outside = (us < -eps) | (us > W - 1 + eps) | (vs < -eps) | (vs > H - 1 + eps)
    assert cov[inside].all() and not cov[outside].any()
    assert (ix[cov] <= W - 2).all() and (iy[cov] <= H - 2).all() and ix.min() >= 0 and iy.min() >= 0
    words = rt.map_words(W, H, K, D, Ko)
    assert words.dtype == np.uint32 and not words[~cov].any()
    assert np.array_equal(words[..., 0] >> 31, cov.astype(np.uint32))
    assert np.array_equal(words[..., 0] & 63, a) and np.array_equal((words[..., 0] >> 6) & 63, b)
    assert np.array_equal(words[..., 1], iy * W + ix)


def test_truth_coverage_of_the_cameras():
    W, H, K, D, _ = CAMERAS["barrel160"]
    assert rt.covered_count(W, H, K, D) == W * H             # barrel: the sensor sees past the output
    cov = rt.map_parts(*CAMERAS["pincushion160"])[0]
    for v, u in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        assert not cov[v, u]
    assert cov[H // 2, W // 2] and rt.covered_count(*CAMERAS["pincushion160"]) == int(cov.sum()) < W * H
    cov = rt.map_parts(*CAMERAS["wide_ko160"])[0]
    assert not cov[0].any() and not cov[:, 0].any() and not cov[-1].any() and not cov[:, -1].any()
    assert cov[H // 2, W // 2]


@pytest.mark.parametrize("W,H,K", [(160, 120, K160), (97, 53, K97), (2, 2, (3.0, 3.0, 0.7, 0.6, 1000.0))])
def test_truth_is_the_identity_without_distortion(W, H, K):
    cov, ix, iy, a, b = rt.map_parts(W, H, K, (0, 0, 0, 0, 0))
    assert cov.all()
    v, u = np.mgrid[0:H, 0:W]
    # the last column and row select the same pixel through a = 32 / b = 32
    assert np.array_equal(ix * 32 + a, u * 32) and np.array_equal(iy * 32 + b, v * 32)
    assert not a[:, :W - 1].any() and not b[:H - 1].any()
    rng = np.random.default_rng(1)
    d = hostile_depth(W, H)
    c3 = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    c1 = rng.integers(0, 256, size=(H, W, 1), dtype=np.uint8)
    do, co = rt.rectify(d, c3, W, H, K, (0, 0, 0, 0, 0))
    assert np.array_equal(do, d) and np.array_equal(co, c3)
    assert np.array_equal(rt.rectify(None, c1, W, H, K, (0, 0, 0, 0, 0))[1], c1)


def test_truth_depth_gate_by_hand():
    """One pixel between a near and a far surface: steps of T - 1 join, T do
    not; a hole at the nearest tap is copied, a negative too."""
    W, H, K = 4, 3, (5.0, 5.5, 1.6, 1.2, 1000.0)
    parts = [np.zeros((H, W), np.int64) for _ in range(5)]
    parts[0] = np.ones((H, W), bool)
    parts[3][:] = 8                                     # a = 8: the nearest tap is the left one
    parts[1][:] = 1
    n = 2000
    T = int(rt.gate(n))
    assert T == 8 + ((96 * (n >> 4) ** 2) >> 16) == 30
    for step, joins in ((T - 1, True), (T, False), (T + 1, False)):
        d = np.full((H, W), n, np.int16)
        d[:, 2] = n + step
        out = rt.rectify_depth(d, parts)
        want = n + (8 * step * 32 + 512) // 1024 if joins else n
        assert out[0, 0] == want, (step, out[0, 0])
    d = np.full((H, W), n, np.int16)
    d[:, 1] = 0
    assert rt.rectify_depth(d, parts)[0, 0] == 0
    d[:, 1] = -7
    assert rt.rectify_depth(d, parts)[0, 0] == -7
    assert int(rt.gate(500)) == 9 and int(rt.gate(8000)) == 255 and int(rt.gate(32767)) == 255


# -------------------------------------------------------------------- YAML --

def test_yaml_distortion_keys(tmp_path):
    golden = os.path.join(GOLDEN, "astra_camera.yaml")
    D = youth_rectify.parse_distortion_yaml(golden)
    assert D is not None and D.as_tuple() == (0.0, 0.0, 0.0, 0.0, 0.0)
    text = open(golden).read()
    lines = [ln for ln in text.splitlines() if not ln.strip().startswith(("Camera.k", "Camera.p"))]
    full = tmp_path / "full.yaml"
    full.write_text("\n".join(lines + ["Camera.k1: -0.28", "Camera.k2: 0.07", "Camera.p1: 8e-4",
                                       "Camera.p2: -6e-4", "  Camera.k3 : 0.011  # comment", ""]))
    D = youth_rectify.parse_distortion_yaml(str(full))
    assert D.as_tuple() == tuple(np.float32(v) for v in (-0.28, 0.07, 8e-4, -6e-4, 0.011))
    part = tmp_path / "part.yaml"
    part.write_text("\n".join(lines + ["Camera.k1: 0.5", "Camera.p2: 0.25", ""]))
    assert youth_rectify.parse_distortion_yaml(str(part)).as_tuple() == (0.5, 0.0, 0.0, 0.25, 0.0)
    assert youth_rectify.parse_distortion_yaml(str(tmp_path / "none.yaml")) is None
    # the old parser reads what it read, whatever the distortion keys say
    want = youth_icp.parse_camera_yaml(golden)
    assert (want[0].as_tuple(), want[1], want[2]) == ((np.float32(570.3), np.float32(570.3), 320.0, 240.0,
                                                       1000.0), 640, 480)
    for p in (full, part):
        got = youth_icp.parse_camera_yaml(str(p))
        assert got[0].as_tuple() == want[0].as_tuple() and got[1:] == want[1:]


# ------------------------------------------------------ the distorted source --

def _inverse_f64(W, H, K, D):
    """youth_synth.h's inverse in numpy: (x, y, closes)."""
    fx, fy, cx, cy, _ = [float(np.float32(v)) for v in K]
    k1, k2, p1, p2, k3 = [float(np.float32(v)) for v in D]
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    xd, yd = (u - cx) / fx, (v - cy) / fy

    def model(x, y):
        r2 = x * x + y * y
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        xy = x * y
        return (rad, (2.0 * p1) * xy + p2 * (r2 + 2.0 * (x * x)),
                p1 * (r2 + 2.0 * (y * y)) + (2.0 * p2) * xy)

    x, y = xd.copy(), yd.copy()
    with np.errstate(all="ignore"):
        for _ in range(30):
            rad, tx, ty = model(x, y)
            x, y = (xd - tx) / rad, (yd - ty) / rad
        rad, tx, ty = model(x, y)
        closes = (np.abs(x * rad + tx - xd) <= 1e-9) & (np.abs(y * rad + ty - yd) <= 1e-9)
    return x, y, closes


def test_distorted_render():
    W, H = 160, 120
    K = intr(K160)
    _, T_wc = youth_synth.sequence(7, 1, W, H, K=K)
    for flags, seed in ((youth_synth.DEFAULT_FLAGS, 11), (youth_synth.SURVEY_FLAGS, 5), (0, 0)):
        d0, c0 = youth_synth.render_rgb(T_wc[0], W, H, K, seed, flags)
        d1, c1 = youth_synth.render_distorted_rgb(T_wc[0], W, H, K, (0, 0, 0, 0, 0), seed, flags)
        assert d0.tobytes() == d1.tobytes() and c0.tobytes() == c1.tobytes()
    ideal_d, ideal_c = youth_synth.render_rgb(T_wc[0], W, H, K, 0, 0)
    for D in (D_BARREL, D_PINCUSHION, (0.9, 0.0, 0.0, 0.0, 0.0)):
        x, y, closes = _inverse_f64(W, H, K160, D)
        d, c = youth_synth.render_distorted_rgb(T_wc[0], W, H, K, D, 0, 0)
        # inside the closed room every ray that exists hits a textured surface
        assert np.array_equal(c.any(axis=-1), closes), D
        assert not d[~closes].any()
        if D == (0.9, 0.0, 0.0, 0.0, 0.0):
            continue
        assert closes.all()
        # the rectifier undoes it: the ideal render, up to resampling
        rd, rc = rt.rectify(d, c, W, H, K160, D)
        cov = rt.map_parts(W, H, K160, D)[0]
        both = cov & (rd > 0) & (ideal_d > 0)
        diff = np.abs(rd.astype(np.int64) - ideal_d)[both]
        cdiff = np.abs(rc.astype(np.int64) - ideal_c)[cov]
        print(D, "depth diff median / 95 %", np.median(diff), np.percentile(diff, 95),
              "colour diff median", np.median(cdiff))
        # two roundings to the millimetre and a bilinear tap: the median pixel
        # lies on a smooth surface
        assert np.median(diff) <= 1 and np.median(cdiff) <= 4


# --------------------------------------------------------------------- ABI --

def test_header_compiles_and_symbols_are_exported():
    src = '#include "youth_rectify.h"\n#include "youth_synth.h"\nint main(void){return 0;}\n'
    inc = os.path.join(ROOT, "include")
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++11")):
        r = subprocess.run([cc, std, "-Wall", "-Werror", "-fsyntax-only", "-I", inc, "-x",
                            "c" if cc == "gcc" else "c++", "-"], input=src, text=True, capture_output=True)
        assert r.returncode == 0, r.stderr
    names = youth_icp.declared_functions(youth_rectify.HEADER_PATH)
    assert len(names) == 10, names
    lib = ctypes.CDLL(os.path.join(PKG, "libyouth_icp.so"))
    for n in names:
        getattr(lib, n)
    getattr(ctypes.CDLL(os.path.join(PKG, "libyouth_synth.so")), "youth_synth_render_distorted_rgb")


_NULL_SWEEP = r"""
import ctypes, re, sys
text = open(sys.argv[1]).read()
text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
text = re.sub(r"typedef[^;]*;", "", text)
lib = ctypes.CDLL(sys.argv[2])
for ret, name, args in re.findall(r"\n\s*([A-Za-z_][\w ]*?\**)\s*\b(youth_\w+)\(([^;{]*)\)\s*;", text):
    ret = ret.strip()
    args = " ".join(args.split())
    n = 0 if args in ("", "void") else args.count(",") + 1
    f = getattr(lib, name)
    f.restype = (None if ret == "void" else ctypes.c_longlong if ret.startswith("long long")
                 else ctypes.c_void_p if ret.endswith("*") else ctypes.c_int)
    f.argtypes = [ctypes.c_void_p] * n
    print(name, ret, f(*([None] * n)), flush=True)
lib.youth_rectify_last_error.restype = ctypes.c_char_p
print("text", len(lib.youth_rectify_last_error() or b""))
"""


def test_null_arguments_are_refused_not_dereferenced(tmp_path):
    """Every function of youth_rectify.h called with NULL / zero for all of its
    arguments, in a child process: an error or an empty answer, no crash, and
    no device is needed to say so."""
    script = tmp_path / "sweep.py"
    script.write_text(_NULL_SWEEP)
    r = subprocess.run([sys.executable, str(script), youth_rectify.HEADER_PATH,
                        os.path.join(PKG, "libyouth_icp.so")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = {}
    for line in r.stdout.splitlines():
        name, *_, val = line.split()
        res[name] = val
    assert len(res) == 11, sorted(res)
    einval = str(youth_icp.YOUTH_EINVAL)
    for n in ("youth_rectify_create", "youth_rectify_map_device", "youth_rectify_device",
              "youth_rectify_host", "youth_rectify_host_frames"):
        assert res[n] == einval, (n, res[n])
    for n in ("youth_parse_camera_yaml_distortion", "youth_rectify_covered", "youth_slam_rectify_active"):
        assert res[n] == "0", (n, res[n])
    assert res["youth_rectify_destroy"] == "None" and int(res["text"]) > 0


def test_create_refuses_bad_arguments_before_the_device():
    """Argument errors do not need a device: each is YOUTH_EINVAL with a text."""
    lib = youth_rectify.load_library()
    K = intr(K160)
    nan = float("nan")
    cases = [
        (160, 120, K, (nan, 0, 0, 0, 0), None),
        (160, 120, K, (0, 0, 0, float("inf"), 0), None),
        (1, 120, K, D_BARREL, None),
        (160, 1, K, D_BARREL, None),
        (16385, 120, K, D_BARREL, None),
        (160, 120, K, D_BARREL, intr((100.0, 100.0, 80.0, 60.0, 5000.0))),
        (160, 120, intr((0.0, 142.0, 80.0, 60.0, 1000.0)), D_BARREL, None),
    ]
    for k, (W, H, Kc, D, Ko) in enumerate(cases):
        with pytest.raises(youth_icp.IcpError) as e:
            youth_rectify.Rectifier(W, H, Kc, D, Ko)
        assert e.value.code == youth_icp.YOUTH_EINVAL, k
        assert (lib.youth_rectify_last_error() or b"").decode().strip(), k


# ------------------------------------------------- the value of the feature --

def _pose_error(T, T_gt):
    R = T[:3, :3] @ T_gt[:3, :3].T
    ang = np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))
    return float(ang), float(np.linalg.norm(T[:3, 3] - T_gt[:3, 3]) * 1000.0)


def value_frames(D, n=16):
    """n consecutive C5 poses rendered through the lens D at 160x120 under
    K160 with DEFAULT_FLAGS -> (depth [n][H][W], rgb [n][H][W][3], T_wc)."""
    W, H = 160, 120
    K = intr(K160)
    _, T_wc = youth_synth.sequence(0, n, W, H, K=K)
    out = [youth_synth.render_distorted_rgb(T_wc[k], W, H, K, D, 1000 + k, youth_synth.DEFAULT_FLAGS)
           for k in range(n)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), T_wc


def test_rectified_frames_track_like_ideal_ones():
    """The three errors of DESIGN.md §17 at the last of sixteen frames: the
    rectified frames track within 4 x the ideal frames' error (rounded up),
    the raw distorted frames do not."""
    K = intr(K160)
    ideal_d, ideal_c, T_wc = value_frames((0, 0, 0, 0, 0))
    raw_d, raw_c, _ = value_frames(D_BARREL)
    rect_d, rect_c = rt.rectify(raw_d, raw_c, 160, 120, K160, D_BARREL)
    T_gt = np.linalg.inv(T_wc[0]) @ T_wc[-1]

    def track(d, c):
        gray = [rgbd_truth.luma(f) for f in c]
        acc = np.eye(4)
        for k in range(1, len(d)):
            acc = acc @ rgbd_truth.align(d[k], gray[k], d[k - 1], gray[k - 1], K, lam=0.1)[0]
        return _pose_error(acc, T_gt)

    e_ideal, e_raw, e_rect = track(ideal_d, ideal_c), track(raw_d, raw_c), track(rect_d, rect_c)
    print(f"e_ideal {e_ideal[0]:.4f} deg {e_ideal[1]:.3f} mm, e_raw {e_raw[0]:.4f} deg {e_raw[1]:.3f} mm, "
          f"e_rect {e_rect[0]:.4f} deg {e_rect[1]:.3f} mm")
    assert 4 * e_ideal[0] <= VALUE_ROT_DEG and 4 * e_ideal[1] <= VALUE_TRANS_MM    # the bound is 4 x this
    assert e_rect[0] <= VALUE_ROT_DEG and e_rect[1] <= VALUE_TRANS_MM
    assert e_raw[0] > VALUE_ROT_DEG and e_raw[1] > VALUE_TRANS_MM
