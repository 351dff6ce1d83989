"""RoadEstimation::HoughLines (the host transform behind RoadEstimation::Compute and the fallback of ComputeBatch)
against tests/hough_reference.py, a float64 restatement of the standard Hough transform with bounds for the votes
whose fp32 rounding float64 cannot predict.  OpenCV itself is not available to compare with; the reference is
written from the transform's definition and shares no code with the implementation.

  * exact frames: seeded images in which the reference finds no ambiguous vote -- there the list must equal the
    reference's bit for bit;
  * full-size frames: every reported line a possible peak, every certain peak reported, the order inside the bounds;
  * the line that decides the road: where one certain peak outvotes every other possible peak, the road parameters
    of the implementation's list equal those of the reference's list, bit for bit (RoadEstimation::ChooseLine);
  * degenerate images.

Every fixture property (no ambiguous vote, equal-vote peaks, the best line at the first / last angle, the
dominant line) is asserted from the reference alone before the implementation is looked at, so no frame passes
by dropping out.  The seeds below were found by a search with the reference alone."""
import numpy as np
import pytest

from hough_reference import THETA, Hough
from instance_stixels_amd import host, make_config

THRESHOLD = 25      # RoadEstimation's accumulator threshold


def vdisp_frame(rows, D, seed, runs=3, noise=4e-4, thick=1):
    """A binary v-disparity image like the road estimation's: the ground ramp d = alpha * (row - v0) below the
    horizon row v0 (synthetic.py's ground, alpha_ground * (v - vhor)), `runs` vertical runs (objects: one
    disparity over a range of rows, each shorter than a third of the ramp) and sparse noise.  Row 0 and column 0
    stay empty."""
    rng = np.random.default_rng(seed)
    img = np.zeros((rows, D), np.uint8)
    v0 = int(rng.integers(rows // 4, rows // 2))
    alpha = float(rng.uniform(0.5, 0.95)) * (D - 1) / (rows - 1 - v0)
    r = np.arange(v0, rows)
    for t in range(thick):
        c = np.rint(alpha * (r - v0)).astype(int) + t
        keep = (c >= 1) & (c < D)
        img[r[keep], c[keep]] = 255
    for _ in range(runs):
        length = int(rng.integers(rows // 16, max(rows // 16 + 1, (rows - v0) // 3)))
        top = int(rng.integers(1, rows - length))
        img[top:top + length, int(rng.integers(1, D))] = 255
    img[rng.random((rows, D)) < noise] = 255
    img[0, :] = 0
    img[:, 0] = 0
    return img


def tie_frame(rows, D, c1, c2, top, length):
    """Mirror-symmetric content -- two equal vertical runs, two equal horizontal runs: peaks with equal votes."""
    img = np.zeros((rows, D), np.uint8)
    img[top:top + length, c1] = 255
    img[top:top + length, c2] = 255
    img[top - 6, 2:2 + length] = 255
    img[top + length + 6, 2:2 + length] = 255
    return img


def first_angle_frame(rows, D, col, seed):
    """A vertical run over nearly all rows beside a ramp: the best line sits at n = 0, next to the zero border."""
    img = vdisp_frame(rows, D, seed, runs=0, noise=0.0)
    img[2:rows - 2, col] = 255
    return img


def last_angle_frame(rows, D, rho_t):
    """The digital line j * cos(a) + i * sin(a) = rho_t for a = 179 degrees: the best line sits at
    n = numangle - 1, next to the zero border on the other side."""
    a = np.deg2rad(179.0)
    img = np.zeros((rows, D), np.uint8)
    i = np.arange(1, rows)
    img[i, np.rint((rho_t - i * np.sin(a)) / np.cos(a)).astype(int)] = 255
    return img


EXACT_FRAMES = (
    [("small-%d" % s, lambda s=s: vdisp_frame(64, 32, s, runs=4, thick=2)) for s in (30, 35, 42, 43)]
    + [("mid-%d" % s, lambda s=s: vdisp_frame(128, 48, s)) for s in (16, 27, 30, 36)]
    + [("medium-%d" % s, lambda s=s: vdisp_frame(256, 64, s)) for s in (614, 756, 2617, 5743)]
    + [("ties", lambda: tie_frame(64, 32, 5, 14, 16, 28)),
       ("first-angle", lambda: first_angle_frame(96, 40, 7, 1)),
       ("last-angle", lambda: last_angle_frame(64, 32, -22))])
FULL_FRAMES = [(rows, D, seed) for rows, D in ((1024, 128), (2048, 256), (784, 128)) for seed in (1, 2, 3)]
# full-size frames whose best line passes the pitch gate and is dominant (in 2048 x 256 seeds 1 and 2 a vertical
# run outvotes the ramp: they stay in FULL_FRAMES)
DOMINANT_FRAMES = ([(1024, 128, s) for s in (1, 2, 3)] + [(2048, 256, s) for s in (3, 4, 9)]
                   + [(784, 128, s) for s in (1, 2, 3)])


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _implementation(img):
    return host.hough_lines(img, rho=1.0, theta=float(THETA), threshold=THRESHOLD, cap=1 << 16)


def _camera(rows):
    cfg = make_config("drn_d_22_unary", 1024, 2048, 128)
    return cfg.camera_center_y * rows / 1024, cfg.baseline, cfg.focal


def assert_exact(h, got):
    want = h.lines()[0]
    assert len(got) == len(want), (len(got), len(want))
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:4].tolist()


def test_angle_step_is_the_one_in_use():
    """The reference's THETA, the default of host.hough_lines and RoadEstimation.cpp's kPi / 180 are one fp32."""
    assert np.float32(np.pi / 180).view(np.int32) == THETA.view(np.int32)
    assert Hough(np.zeros((8, 8), np.uint8)).numangle == 180


@pytest.mark.parametrize("name", [n for n, _ in EXACT_FRAMES])
def test_exact_frames(name):
    img = dict(EXACT_FRAMES)[name]()
    h = Hough(img, threshold=THRESHOLD)
    assert h.n_ambiguous == 0 and h.n_points > THRESHOLD, "the fixture is no longer an exact frame"
    want, n, r, votes = h.lines()
    assert len(want) >= 1
    print(f"{name}: {img.shape} points {h.n_points} lines {len(want)} best (n {n[0]}, r {r[0]}, votes {votes[0]})")
    if name == "ties":
        assert votes[0] == votes[1] == votes[2] and (np.diff(votes) == 0).sum() >= 3
    if name == "first-angle":
        assert n[0] == 0 and votes[0] > votes[1]
    if name == "last-angle":
        assert n[0] == h.numangle - 1 and votes[0] > votes[1]
    got = _implementation(img)
    assert_exact(h, got)
    h.check_lines(got)


def _dominant_road(h, got, rows):
    """Test 3: asserts the condition on the input from the reference alone, then the road parameters."""
    cam = _camera(rows)
    want, n, r, _ = h.lines()
    k, road = host.choose_line(want, *cam, rows)
    assert k >= 0 and h.dominant(n[k], r[k]), "the fixture has no dominant line that passes the pitch gate"
    k_got, road_got = host.choose_line(got, *cam, rows)
    assert k_got >= 0 and np.array_equal(_bits(got[k_got]), _bits(want[k]))
    assert road_got[0] == road[0] and np.array_equal(_bits(road_got[1:]), _bits(road[1:])), (road_got, road)


@pytest.mark.parametrize("rows,D,seed", FULL_FRAMES)
def test_full_size_frames(rows, D, seed):
    img = vdisp_frame(rows, D, seed, runs=6, thick=2)
    h = Hough(img, threshold=THRESHOLD)
    certain, possible = int(h.certain_peaks().sum()), int(h.possible_peaks().sum())
    print(f"{rows}x{D} seed {seed}: points {h.n_points} ambiguous {h.n_ambiguous} of {h.n_votes} votes, "
          f"certain peaks {certain}, possible peaks {possible}")
    assert h.n_ambiguous > 0 and certain >= 10
    got = _implementation(img)
    assert certain <= len(got) <= possible
    h.check_lines(got)


@pytest.mark.parametrize("rows,D,seed", DOMINANT_FRAMES)
def test_deciding_line_on_full_size_frames(rows, D, seed):
    img = vdisp_frame(rows, D, seed, runs=6, thick=2)
    _dominant_road(Hough(img, threshold=THRESHOLD), _implementation(img), rows)


# (not among them: small-30, whose two best lines tie, and the three hand-made frames, whose best line is none
# the pitch gate accepts or none that stands alone)
@pytest.mark.parametrize("name", [n for n, _ in EXACT_FRAMES
                                  if n not in ("small-30", "ties", "first-angle", "last-angle")])
def test_deciding_line_on_exact_frames(name):
    img = dict(EXACT_FRAMES)[name]()
    _dominant_road(Hough(img, threshold=THRESHOLD), _implementation(img), img.shape[0])


def _degenerate(name):
    img = np.zeros((32, 16) if name == "every-pixel" else (64, 32), np.uint8)
    if name == "one-pixel":
        img[40, 9] = 255
    elif name == "below-threshold":
        img[10:10 + THRESHOLD, 8] = 255             # a run of exactly `threshold` pixels: v > threshold fails
    elif name == "above-threshold":
        img[10:10 + THRESHOLD + 1, 8] = 255
    elif name == "every-pixel":
        img[:] = 255
    elif name == "full-row":
        img[6, :] = 255
    elif name == "full-column":
        img[:, 8] = 255
    return img


@pytest.mark.parametrize("name,exact,n_lines", [
    ("all-zero", True, 0), ("one-pixel", True, 0), ("below-threshold", True, 0), ("above-threshold", True, None),
    ("every-pixel", False, None), ("full-row", True, None), ("full-column", True, None)])
def test_degenerate_images(name, exact, n_lines):
    img = _degenerate(name)
    h = Hough(img, threshold=THRESHOLD)
    certain, possible = int(h.certain_peaks().sum()), int(h.possible_peaks().sum())
    print(f"{name}: points {h.n_points} ambiguous {h.n_ambiguous}, certain peaks {certain}, possible {possible}")
    assert (h.n_ambiguous == 0) == exact, "the fixture changed its kind"
    if n_lines is None:
        assert certain >= 1
    else:
        assert possible == n_lines
    got = _implementation(img)
    assert certain <= len(got) <= possible
    h.check_lines(got)
    if exact:
        assert_exact(h, got)
