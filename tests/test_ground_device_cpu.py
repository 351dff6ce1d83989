"""The host half of the device-resident road chain, without a GPU:

  * is_erff / is_atanf / is_cosf (include/is_numerics.h, through the host library) against float64 numpy / scipy
    rounded to float32 -- within 1 ulp, the C99 special values, oddness, monotonicity, the saturation point;
  * Stixels::PrecomputeGroundShared (the twin of k_ground_model) against the legacy Stixels::PrecomputeGround;
  * RoadEstimation::ChooseLineShared (the twin of k_road_choose) against the legacy RoadEstimation::ChooseLine;
  * the same host code with hostile lines and roads in a stand-alone program under UBSan + ASan.

tests/ground_reference.py restates PrecomputeGround in numpy fp32 with the erf left open; it is pinned bitwise against
both C++ functions first, and then supplies the FastLog indices neither of them shows."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.special

import ground_reference as gr
import helpers
from hough_reference import THETA
from instance_stixels_amd import core, host, make_config
from test_hough_reference import DOMINANT_FRAMES, EXACT_FRAMES, FULL_FRAMES, _camera, vdisp_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _ordered(x):
    """fp32 values as integers in the order of the reals (+-0 both 0): differences count ulps"""
    b = _bits(x).astype(np.int64)
    return np.where(b < 0, -(b & 0x7fffffff), b)


def _ulps(a, b):
    return np.abs(_ordered(a) - _ordered(b))


def _run(x, n):
    """the n floats below x, x, and the n floats above it"""
    i = int(np.float32(x).view(np.int32))
    return np.arange(i - n, i + n + 1, dtype=np.int32).view(np.float32)


def _round32(f64):
    with np.errstate(over="ignore", under="ignore"):
        return np.asarray(f64, np.float64).astype(np.float32)


# ---------------------------------------------------------------- the shared functions

ERF_BOUNDARIES = [k / 4 for k in range(1, 17)]   # the pieces of is_erff: [k/4, (k+1)/4), +-1 from 4 on


def _erf_points():
    rng = np.random.default_rng(11)
    pts = [np.linspace(-6, 6, 120001), rng.uniform(-6, 6, 60000), rng.normal(0, 0.3, 20000)]
    pts += [_run(b, 64) for b in ERF_BOUNDARIES] + [-_run(b, 64) for b in ERF_BOUNDARIES]
    pts += [10.0 ** rng.uniform(-45, -1, 4000), -(10.0 ** rng.uniform(-45, -1, 4000))]   # down to the subnormals
    pts += [np.array([1e-45, 1.1754944e-38, 1.1754942e-38, 3e-39], np.float32)]
    return np.concatenate([np.asarray(p, np.float32) for p in pts])


def test_is_erff_is_within_one_ulp_of_float64_erf():
    x = _erf_points()
    assert x.size >= 100000
    got = host.is_erff(x)
    want = _round32(scipy.special.erf(x.astype(np.float64)))
    d = _ulps(got, want)
    print(f"is_erff: {x.size} points, {int((d > 0).sum())} differ from the rounded float64 erf, worst {int(d.max())} ulp")
    assert d.max() <= 1, x[np.argmax(d)]
    assert (np.abs(got) <= 1).all()


def test_is_erff_special_values_and_symmetry():
    sp = host.is_erff(np.array([0.0, -0.0, np.inf, -np.inf, 4.0, -4.0, 3.4e38], np.float32))
    assert np.array_equal(_bits(sp), _bits([0.0, -0.0, 1.0, -1.0, 1.0, -1.0, 1.0]))
    assert np.isnan(host.is_erff(np.array([np.nan, -np.nan], np.float32))).all()
    x = np.abs(_erf_points())
    assert np.array_equal(_bits(host.is_erff(-x)), _bits(-host.is_erff(x)))   # odd, bit for bit


def test_is_erff_is_monotone_and_saturates_where_erff_does():
    x = np.sort(_erf_points())
    assert (np.diff(host.is_erff(x)) >= 0).all()
    # every float of [3.5, 4.125): the last pieces, the point where the value becomes 1, the hand-over at 4
    lo, hi = np.float32(3.5).view(np.int32), np.float32(4.125).view(np.int32)
    x = np.arange(lo, hi, dtype=np.int32).view(np.float32)
    got = host.is_erff(x)
    assert (np.diff(got) >= 0).all() and got[-1] == 1.0 and got[0] < 1.0
    want = _round32(scipy.special.erf(x.astype(np.float64)))
    assert _ulps(got, want).max() <= 1
    first = x[np.argmax(got == 1.0)]
    # libm on every float from 1000 below that point up to 4.125: wherever erff is 1, is_erff is 1
    k = max(int(np.argmax(got == 1.0)) - 1000, 0)
    libm = gr.libm_erff(x[k:])
    print(f"is_erff == 1 from {first!r} on; erff == 1 from {x[k:][np.argmax(libm == 1.0)]!r} on")
    assert (got[k:][libm == 1.0] == 1.0).all()
    assert (host.is_erff(-x[k:])[libm == 1.0] == -1.0).all()
    assert got[int(np.argmax(got == 1.0)):].min() == 1.0   # and it stays there


def test_is_atanf_is_within_one_ulp_and_follows_c99():
    rng = np.random.default_rng(12)
    mag = 10.0 ** np.concatenate([np.linspace(-30, 30, 60001), rng.uniform(-30, 30, 40000)])
    pieces = np.concatenate([_run(k / 8, 64) for k in range(1, 9)] + [_run(1.0, 200)])
    x = np.concatenate([mag, -mag, pieces, -pieces, np.linspace(-4, 4, 40001)]).astype(np.float32)
    got = host.is_atanf(x)
    d = _ulps(got, _round32(np.arctan(x.astype(np.float64))))
    print(f"is_atanf: {x.size} points, {int((d > 0).sum())} differ from the rounded float64 atan, worst {int(d.max())} ulp")
    assert d.max() <= 1, x[np.argmax(d)]
    assert _ulps(got[:2000], gr.libm_atanf(x[:2000])).max() <= 1   # and libm itself on a sample
    half_pi = np.float32(np.pi / 2)
    sp = host.is_atanf(np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45], np.float32))
    assert np.array_equal(_bits(sp), _bits([0.0, -0.0, half_pi, -half_pi, 1e-45, -1e-45]))
    assert np.isnan(host.is_atanf(np.array([np.nan], np.float32))).all()
    assert np.array_equal(_bits(host.is_atanf(-x)), _bits(-got))
    xs = np.sort(x)
    assert (np.diff(host.is_atanf(xs)) >= 0).all()


def test_is_cosf_is_within_one_ulp_on_the_range_of_is_atanf():
    half_pi = np.float32(np.pi / 2)
    rng = np.random.default_rng(13)
    x = np.concatenate([np.linspace(-np.pi / 2, np.pi / 2, 120001), rng.uniform(-np.pi / 2, np.pi / 2, 40000),
                        _run(np.pi / 4, 200), -_run(np.pi / 4, 200),
                        np.arange(half_pi.view(np.int32) - 4000, half_pi.view(np.int32) + 1, dtype=np.int32).view(np.float32),
                        half_pi - 10.0 ** np.linspace(-7, -1, 2000), [0.0, -0.0, 1e-45, 1e-30]]).astype(np.float32)
    x = x[np.abs(x) <= half_pi]
    got = host.is_cosf(x)
    d = _ulps(got, _round32(np.cos(x.astype(np.float64))))
    print(f"is_cosf: {x.size} points, {int((d > 0).sum())} differ from the rounded float64 cos, worst {int(d.max())} ulp")
    assert d.max() <= 1, x[np.argmax(d)]
    assert _ulps(got[::97], gr.libm_cosf(x[::97])).max() <= 1
    assert np.isnan(host.is_cosf(np.array([np.nan], np.float32))).all()
    assert np.array_equal(_bits(host.is_cosf(-x)), _bits(got))
    # the pitch of every line is an is_atanf: its range lies in the domain covered above
    assert abs(float(host.is_atanf(np.array([np.inf], np.float32))[0])) <= half_pi


def test_the_header_holds_what_the_generator_prints():
    pytest.importorskip("mpmath")
    subprocess.run(["python3", os.path.join(ROOT, "tools", "gen_is_numerics.py"), "--check"], check=True)


# ---------------------------------------------------------------- the ground model

SHAPES = [(256, 512, 64), (1024, 2048, 128)]
MAX_DIFFERING_ROWS = 0.005   # share of a frame's rows whose FastLog index may differ from the legacy model's


def _stixels(cfg):
    st = host.Stixels()
    st.SetConfig(cfg)
    st.PrecomputeHost()
    return st


def _roads(shape):
    """the roads of helpers.build_case's 8 frames, and 24 seeded roads around them (horizon, tilt, height, slope)"""
    rows, cols, D = shape
    case = helpers.build_case("drn_d_22_unary", rows, cols, D, seed=5, n_images=8)
    roads = [(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground) for f in case["frames"]]
    rng = np.random.default_rng(rows)
    v0, _, _, a0 = roads[0]
    for _ in range(24):
        roads.append((int(rng.integers(rows // 4, 3 * rows // 4)), float(rng.uniform(-0.1, 0.1)),
                      float(rng.uniform(1.0, 2.2)), float(a0 * rng.uniform(0.6, 1.5))))
    return case["cfg"], roads


@pytest.mark.parametrize("shape", SHAPES)
def test_shared_ground_model_against_the_legacy_one(shape):
    rows = shape[0]
    cfg, roads = _roads(shape)
    st = _stixels(cfg)
    gp, lut = st.GroundParams(), st.GetLogLUT()
    assert lut.size == gr.LOG_LUT_SIZE + 1
    worst, total, total_case = 0, 0, 0
    for i, (vhor_image, tilt, height, alpha) in enumerate(roads):
        st.SetRoadParameters(vhor_image, tilt, height, alpha)
        l_fn, l_norm, l_is2, vhor_lib = st.GetGroundModel()                              # legacy
        s_fn, s_norm, s_is2, s_idx = st.PrecomputeGroundShared(vhor_lib, tilt, height, alpha)
        assert vhor_lib == rows - vhor_image - 1
        # the restatement is both functions, bit for bit, once the erf is chosen
        legacy = gr.precompute_ground(gp, lut, rows, vhor_lib, tilt, height, alpha, gr.libm_erff)
        shared = gr.precompute_ground(gp, lut, rows, vhor_lib, tilt, height, alpha, host.is_erff)
        assert legacy["in_range"].all() and shared["in_range"].all(), i
        for got, want in ((l_fn, legacy["function"]), (l_norm, legacy["normalization"]), (l_is2, legacy["inv_sigma2"]),
                          (s_fn, shared["function"]), (s_norm, shared["normalization"]), (s_is2, shared["inv_sigma2"])):
            assert np.array_equal(_bits(got), _bits(want)), i
        assert np.array_equal(s_idx, shared["idx_range"]), i
        # what holds no transcendental is equal
        assert np.array_equal(_bits(s_fn), _bits(l_fn)) and np.array_equal(_bits(s_is2), _bits(l_is2)), i
        assert np.array_equal(shared["idx_pout"], legacy["idx_pout"]), i
        # the rest: equal wherever the indices agree, which differ by at most 1 and in few rows
        same = shared["idx_range"] == legacy["idx_range"]
        assert np.array_equal(_bits(s_norm[same]), _bits(l_norm[same])), i
        assert np.abs(shared["idx_range"] - legacy["idx_range"]).max() <= 1, i
        differing = int((~same).sum())
        assert differing <= MAX_DIFFERING_ROWS * rows, (i, differing)
        worst, total = max(worst, differing), total + differing
        total_case += differing if i < 8 else 0
        assert np.isneginf(s_norm[vhor_lib:]).any()    # rows at and above the horizon: FastLog(0) = -inf
    print(f"{shape}: the FastLog index differs from the legacy model's in {total_case} of {8 * rows} rows of "
          f"build_case's 8 roads and in {total} of {len(roads) * rows} rows of all {len(roads)} roads "
          f"({100.0 * total / (len(roads) * rows):.4f} %); worst frame {worst} of {rows} rows")
    st.close()


def test_shared_ground_model_is_defined_for_any_road():
    """The clamped FastLog index: degenerate roads (height 0, NaN, inf, a horizon far outside) give numbers or NaN,
    never an index outside the table -- the device reads d_road from memory a caller filled."""
    cfg = make_config("drn_d_22_unary", 256, 512, 64)
    st = _stixels(cfg)
    for road in ((0, 0.0, 0.0, 0.0), (-2**31, np.nan, np.nan, np.nan), (2**31 - 1, np.inf, -np.inf, np.inf),
                 (100, 0.01, 1e-30, 3e38), (100, -1.0, -1.5, -0.3), (100, 0.0, 1.5, 1e-45)):
        fn, norm, is2, idx = st.PrecomputeGroundShared(*road)
        assert idx.min() >= 0 and idx.max() <= gr.LOG_LUT_SIZE, road
    st.close()


# ---------------------------------------------------------------- the line choice

def _line_lists():
    out = [(name, make()) for name, make in EXACT_FRAMES]
    out += [(f"full-{rows}x{D}-{seed}", vdisp_frame(rows, D, seed, runs=6, thick=2))
            for rows, D, seed in sorted(set(FULL_FRAMES + DOMINANT_FRAMES))[::2]]
    return out


@pytest.fixture(scope="module")
def line_lists():
    return [(name, img.shape[0], host.hough_lines(img, rho=1.0, theta=float(THETA), threshold=25, cap=1 << 16))
            for name, img in _line_lists()]


def test_choose_line_shared_against_choose_line(line_lists):
    accepted = 0
    for name, rows, lines in line_lists:
        cam = _camera(rows)
        k, road = host.choose_line(lines, *cam, rows)
        fb = (7, 0.5, 1.25, 0.75)
        st, k_s, road_s = host.choose_line_shared(lines, len(lines), 0, max(len(lines), 1), *cam, rows, fallback=fb)
        assert k_s == k, name
        if k < 0:
            assert st == core.ROAD_NONE and road_s == (7, np.float32(0.5), np.float32(1.25), np.float32(0.75)), name
            continue
        if not 0 <= road[0] < rows:
            assert st == core.ROAD_HORIZON and road_s[0] == 7, name
            continue
        accepted += 1
        assert st == core.ROAD_OK, name
        assert road_s[0] == road[0] and _bits(road_s[3]) == _bits(road[3]), (name, road_s, road)   # vhor, alpha
        assert _ulps(road_s[1], road[1]) <= 1 and _ulps(road_s[2], road[2]) <= 2, (name, road_s, road)
        # a truncated list: undecided exactly when the accepted line is cut off
        st_cut, k_cut, road_cut = host.choose_line_shared(lines, len(lines), 0, k + 1, *cam, rows, fallback=fb)
        assert (st_cut, k_cut, road_cut) == (st, k_s, road_s), name
        if k > 0:
            st_cut, k_cut, road_cut = host.choose_line_shared(lines, len(lines), 0, k, *cam, rows, fallback=fb)
            assert st_cut == core.ROAD_UNDECIDED and k_cut == -1 and road_cut[0] == 7, name
        st_over, k_over, _ = host.choose_line_shared(lines, len(lines), 1, len(lines), *cam, rows, fallback=fb)
        assert st_over == core.ROAD_UNDECIDED and k_over == -1, name
    print(f"{len(line_lists)} line lists, {accepted} with an accepted line")
    assert accepted >= 10


def test_choose_line_shared_rejects_degenerate_lines():
    rows = 256
    cam = _camera(rows)
    step = np.float32(THETA)
    th = lambda n: np.float32(0.0) + np.float32(n) * step
    fb = (3, 0.25, 1.5, 0.5)
    good = [100.0, th(80)]
    k_good, road_good = host.choose_line(np.array([good], np.float32), *cam, rows)
    assert k_good == 0 and 0 <= road_good[0] < rows
    hostile = [[5.0, th(0)],        # theta = 0: rho / 0 = inf
               [0.0, th(0)],        # 0 / 0
               [np.nan, th(45)], [np.inf, th(45)], [10.0, np.nan], [10.0, 1.0], [10.0, -step], [10.0, th(180)]]
    st, k, road = host.choose_line_shared(np.array(hostile + [good], np.float32), len(hostile) + 1, 0, 64, *cam, rows,
                                          fallback=fb)
    assert (st, k) == (core.ROAD_OK, len(hostile)) and road[0] == road_good[0]
    st, k, road = host.choose_line_shared(np.array(hostile, np.float32), len(hostile), 0, 64, *cam, rows, fallback=fb)
    assert (st, k) == (core.ROAD_NONE, -1) and road == (3, np.float32(0.25), np.float32(1.5), np.float32(0.5))
    # rho = 0 at 90 degrees is a line like any other (horizon in row 0): both choices take it
    zero = np.array([[0.0, th(90)]], np.float32)
    k_l, road_l = host.choose_line(zero, *cam, rows)
    st, k, road = host.choose_line_shared(zero, 1, 0, 64, *cam, rows, fallback=fb)
    assert (k_l, road_l[0]) == (0, 0) and (st, k, road[0]) == (core.ROAD_OK, 0, 0)
    # a line whose pitch passes and whose horizon lies far outside the image: flagged, the fallback in place
    cy, b, f = cam
    far = [np.float32((cy + 0.9 * f) * np.sin(np.float64(th(90)))), th(90)]
    st, k, road = host.choose_line_shared(np.array([far], np.float32), 1, 0, 64, *cam, rows, fallback=fb)
    assert (st, k) == (core.ROAD_HORIZON, 0) and road[0] == 3


SANITIZE_SRC = os.path.join(ROOT, "tests", "sanitize", "ground_device_main.cpp")


def test_host_twins_under_ubsan_and_asan(tmp_path):
    """The stand-alone program (its own main) over the host code of the chain -- RoadEstimation::ChooseLineShared on
    hostile line lists, is_ground_row on hostile roads -- built with -fsanitize=undefined,address and run once."""
    cxx = shutil.which("g++")
    assert cxx is not None, "the build needs g++ too"
    lib_dir = os.path.join(ROOT, "instance_stixels_amd", "lib")
    exe = str(tmp_path / "ground_device_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math",
                    "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "instance_stixels_amd", "host"), SANITIZE_SRC,
                    os.path.join(ROOT, "instance_stixels_amd", "host", "RoadEstimation.cpp"),
                    "-L" + lib_dir, "-lis_core", "-Wl,-rpath," + lib_dir, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True)
    print(r.stdout[-400:], r.stderr[-2000:])
    assert r.returncode == 0 and "ground_device_main: ok" in r.stdout
